"""The approximate k-NN (knn_descent) on the MI355X against its numpy specification (tests/_knn_descent_ref.py), bit for
bit and stage by stage: the start on X, one join on random lists (so the join does all the work), the full run, and the properties the
specification promises -- the exact search's bits for every kept pair, K = n - 1 exact, no dependence on the launch split."""
import ctypes as C
import functools

import numpy as np
import pytest

import _knn_descent_ref as ref

pytestmark = pytest.mark.gpu
RECALL_20011 = 0.998           # the reference's recall on blobs 20 011 x 10, K = 15 (0.99824..., measured once on the CPU)


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


@pytest.fixture(scope="module")
def stages():
    from sharp_amd.tsne import _knn_descent_join, _knn_descent_start

    return _knn_descent_start, _knn_descent_join


@functools.lru_cache(maxsize=None)
def stage_input(d):
    return ref.stage_input(d)


@functools.lru_cache(maxsize=None)
def full_reference(name):
    X = ref.full_input(name)
    return (X,) + ref.descent(X, 15)


def same(got, want):
    assert np.array_equal(got[0], want[0]), f"indices differ in {int((got[0] != want[0]).any(1).sum())} rows"
    assert got[1].dtype == np.float64 and np.array_equal(got[1], want[1]), "squared distances differ in their bits"


# ---- the start alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", (1, 8))
@pytest.mark.parametrize("d,K", ref.STAGE_CASES)
def test_start_equals_the_reference(sa, stages, d, K, T):
    X = stage_input(d)
    got = stages[0](X, K, T, 10)
    want = ref.start(X, K, T, 10)
    same(got, want)
    assert np.array_equal(got[1], ref.pair_dist2(X, np.arange(X.shape[0])[:, None], got[0].astype(np.int64)))   # the direct sum


# ---- one join from given lists --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K", ref.STAGE_CASES + [(d, 1) for d in ref.DS])
def test_one_join_equals_the_reference(sa, stages, d, K):
    X = stage_input(d)
    lists = ref.random_lists(X.shape[0], K, 7 + K)
    gi, gd, gu = stages[1](X, lists, None, 1, 10)
    wi, wd, wu = ref.join(X, ref.lists_of(X, lists)[0], None, 1, 10)
    same((gi, gd), (wi, wd))
    assert gu == wu and gu > 0


@pytest.mark.parametrize("S,iteration,seed", [(5, 3, 4), (40, 2, 10)])
def test_join_honours_candidates_iteration_and_seed(sa, stages, S, iteration, seed):
    X = stage_input(10)
    lists = ref.random_lists(X.shape[0], 15, 5)
    gi, gd, gu = stages[1](X, lists, S, iteration, seed)
    wi, wd, wu = ref.join(X, ref.lists_of(X, lists)[0], S, iteration, seed)
    same((gi, gd), (wi, wd))
    assert gu == wu


@pytest.mark.parametrize("d", (10, 50))
def test_planted_duplicates_come_lower_index_first(sa, stages, d):
    X, lists = ref.planted_duplicates(d)
    gi, gd, gu = stages[1](X, lists, None, 1, 10)
    wi, wd, wu = ref.join(X, ref.lists_of(X, lists)[0], None, 1, 10)
    same((gi, gd), (wi, wd))
    assert gu == wu
    assert gi[3, :2].tolist() == [700, 701] and gd[3, :2].tolist() == [0.0, 0.0]
    assert gi[700, :2].tolist() == [3, 701] and gi[701, :2].tolist() == [3, 700]


# ---- the full run ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.FULL_INPUTS)
def test_full_run_equals_the_reference(sa, stages, name):
    X, wi, wd, winfo = full_reference(name)
    gi, gd, ginfo = sa.knn_descent(X, 15, squared=True, ret_info=True)
    same((gi, gd), (wi, wd))
    assert (ginfo["joins"], ginfo["updates"], ginfo["reason"]) == (winfo["joins"], winfo["updates"], ("n_iters", "delta")[winfo["reason"]])
    assert ginfo["method"] == "descent"
    again = sa.knn(X, 15, squared=True, method="descent")
    same(again, (gi, gd))                                            # two calls, the same bits
    same(sa.knn_descent(X, 15, squared=True, n_iters=0), stages[0](X, 15, 8, 10))
    root = sa.knn(X, 15, method="nndescent")
    assert np.array_equal(root[0], gi) and np.array_equal(root[1], np.sqrt(gd))
    # a run cut short by n_iters says so
    ci, cd, cinfo = sa.knn_descent(X, 15, squared=True, n_iters=1, ret_info=True)
    w1 = ref.join(X, ref.start(X, 15)[0], None, 1, 10)
    same((ci, cd), w1[:2])
    assert (cinfo["joins"], cinfo["updates"], cinfo["reason"]) == (1, w1[2], "n_iters")


def test_K_equal_n_minus_1_is_the_exact_list(sa):
    X = ref.gaussian(256, 7, 5)
    same(sa.knn_descent(X, 255, squared=True), sa.knn(X, 255, squared=True))
    same(sa.knn_descent(X, 255, squared=True, n_projections=1, n_iters=0), sa.knn(X, 255, squared=True))


def test_exact_default_is_untouched(sa):
    X = stage_input(10)
    from sharp_amd.tsne import _knn

    i, d2 = _knn(X, 15)
    same(sa.knn(X, 15, squared=True), (i, d2))
    same(sa.knn(X, 15, squared=True, method="exact"), (i, d2))


# ---- where launches split -------------------------------------------------------------------------------------------------------------
def test_launch_splits_and_the_exact_search_bits(sa, stages):
    X = ref.full_input("blobs20011")
    n, K = X.shape[0], 15
    gi, gd, info = sa.knn_descent(X, K, squared=True, ret_info=True)
    ei, ed = sa.knn(X, K, squared=True)
    both = gi[:, :, None] == ei[:, None, :]
    recall = both.sum() / float(n * K)
    print(f"recall against the exact lists {recall!r}, {info}")
    shape = both.shape
    assert np.array_equal(np.broadcast_to(gd[:, :, None], shape)[both], np.broadcast_to(ed[:, None, :], shape)[both])
    assert recall >= RECALL_20011
    # a forced small rows-per-launch (5 004 rows: four full launches and a ragged one) gives the same bits, stage by stage
    si, sd = stages[0](X, K, 8, 10)
    same(stages[0](X, K, 8, 10, 5004), (si, sd))
    whole = stages[1](X, si, None, 1, 10)
    split = stages[1](X, si, None, 1, 10, 5004)
    same(split[:2], whole[:2])
    assert split[2] == whole[2]


# ---- downstream -----------------------------------------------------------------------------------------------------------------------
def test_maps_from_descent_lists(sa):
    X = ref.blobs(600, 10, 9)
    lists = sa.knn(X, 14, method="descent")
    u = sa.umap_neighbors(*lists, n_epochs=30)
    v = sa.umap(X, nn_method="descent", init="random", n_epochs=30, ret_nn=True)
    assert np.isfinite(u["Y"]).all() and np.array_equal(u["Y"], v["Y"])
    assert np.array_equal(v["nn"]["index"], lists[0]) and np.array_equal(v["nn"]["distance"], lists[1]) and v["nn"]["method"] == "descent"
    assert np.array_equal(sa.umap(X, nn_method="nndescent", init="random", n_epochs=30)["Y"], u["Y"])
    w = sa.umap(X, nn_method="descent", n_epochs=30, nn_args={"n_iters": 1, "seed": 3}, ret_model=True)     # (the PCA start; a model)
    assert np.isfinite(w["Y"]).all() and not np.array_equal(w["Y"], u["Y"])
    with w["model"] as m:
        assert sa.umap_transform(X[:10], m)["Y"].shape == (10, 2)
    sq = sa.knn(X, 30, squared=True, method="descent")
    t = sa.Rtsne_neighbors(*sq, squared=True, perplexity=10, max_iter=20)
    r = sa.Rtsne(X, nn_method="descent", perplexity=10, max_iter=20, pca=False, normalize=False)
    assert np.isfinite(t["Y"]).all() and np.array_equal(t["Y"], r["Y"]) and r["origD"] == 10


def test_visualization_sharp_with_descent(sa, oracle):
    X = oracle.synth_fill(20261003, 1500, 0, 1200, 4, 200)
    res = sa.SHARP(X, rN_seed=2103, ensize_K=3)
    for kw in ({"max_iter": 20}, {"method": "umap", "n_epochs": 20}):
        v = sa.visualization_SHARP(res, plot=False, nn_method="descent", return_neighbors=True, **kw)
        nb = v["neighbors"]
        assert nb["method"] == "descent" and nb["n"] == 1200 and np.isfinite(v["Y"]).all()
        again = sa.visualization_SHARP(res, plot=False, neighbors=nb, **kw)
        assert np.array_equal(again["Y"], v["Y"])
        quiet = sa.visualization_SHARP(res, plot=False, nn_method="descent", **kw)
        assert np.array_equal(quiet["Y"], v["Y"]) and "neighbors" not in quiet
    exact = sa.visualization_SHARP(res, plot=False, max_iter=20, return_neighbors=True)["neighbors"]
    assert "method" not in exact and exact["index"].shape == (1200, 90)      # (the exact search's dict is what it always was)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_leave_the_library_usable(sa, stages):
    E = sa.SharpError
    X = ref.blobs(300, 6, 3)
    want = sa.knn_descent(X, 10, squared=True)

    def good():
        same(sa.knn_descent(X, 10, squared=True), want)

    for rows, K, match in ((300, 0, "K must be in 1 .. 255"), (300, 256, "K must be in 1 .. 255"), (100, 100, "K <= n - 1")):
        with pytest.raises(E, match=match):
            sa.knn_descent(X[:rows], K)
        with pytest.raises(E, match=match):
            sa.knn(X[:rows], K, method="descent")
    for kw, match in (({"n_projections": 0}, "n_projections"), ({"n_projections": 33}, "n_projections"), ({"max_candidates": 0}, "max_candidates"),
                      ({"max_candidates": 256}, "max_candidates"), ({"n_iters": -1}, "n_iters"), ({"delta": -0.1}, "delta"),
                      ({"delta": float("nan")}, "delta"), ({"seed": -1}, "seed"), ({"seed": 0.5}, "seed")):
        with pytest.raises(E, match=match):
            sa.knn_descent(X, 10, **kw)
        good()
    # the library's own checks, behind the package's: the C entry refuses the same things by name
    L = sa.lib()
    idx, d2, info = np.zeros((300, 10), np.int32), np.zeros((300, 10)), np.zeros(4, np.int64)
    P = lambda a: a.ctypes.data                                      # noqa: E731
    for args, match in (((10, 0, 0, 12, 0.001, 10.0), "n_projections"), ((10, 8, 300, 12, 0.001, 10.0), "max_candidates"),
                        ((10, 8, 0, -2, 0.001, 10.0), "n_iters"), ((10, 8, 0, 12, 2.0, 10.0), "delta"), ((0, 8, 0, 12, 0.001, 10.0), "K must be"),
                        ((10, 8, 0, 12, 0.001, 2.0 ** 53), "seed")):
        assert L.sharp_knn_descent(P(X), 300, 6, 6, *args, P(idx), P(d2), P(info)) == 2
        assert match in L.sharp_last_error().decode()
    good()
    for v in (np.nan, np.inf, -np.inf, 1e101):
        bad = X.copy()
        bad[57, 4] = v
        with pytest.raises(E, match=r"NA / NaN / Inf or a value beyond 1e100 \(row 58, column 5\)"):
            sa.knn_descent(bad, 10)
        with pytest.raises(E, match=r"row 58, column 5"):
            stages[0](bad, 10)
        good()
    with pytest.raises(E, match="is_distance"):
        sa.knn(np.abs(X[:, 0]), 3, is_distance=True, method="descent")
    with pytest.raises(E, match="nn_method must be"):
        sa.knn(X, 3, method="annoy")
    with pytest.raises(E, match="belong to method"):
        sa.knn(X, 3, n_iters=2)
    with pytest.raises(E, match="is_distance"):
        sa.Rtsne(np.abs(X[:, 0]), is_distance=True, nn_method="descent")
    with pytest.raises(E, match="nn_method must be"):
        sa.umap(X, nn_method="annoy")
    # a join's given lists are validated before an index is dereferenced
    lists = ref.random_lists(300, 10, 1)
    for value, match in ((300, r"outside \[0, n\) \(row 41,"), (-1, r"outside \[0, n\) \(row 41,"), (41, r"names itself")):
        b = lists.copy()
        b[41, 2] = value
        with pytest.raises(E, match=match):
            stages[1](X, b)
    b = lists.copy()
    b[41, 2] = b[41, 7]
    with pytest.raises(E, match=r"twice in a row \(row 41,"):
        stages[1](X, b)
    good()


# ---- the .C() twin --------------------------------------------------------------------------------------------------------------------
def test_dotc_twin(sa):
    L = sa.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    I = lambda v: np.array([v], np.int32)                            # noqa: E731
    D = lambda v: np.array([v], np.float64)                          # noqa: E731
    X = ref.blobs(600, 10, 9)
    n, K = 600, 14
    idx, d2, info, st = np.zeros((n, K), np.int32), np.zeros((n, K)), np.zeros(4), I(-1)
    L.sharp_C_knn_descent(*[P(v) for v in (X, D(n), I(10), I(K), I(4), I(20), I(3), D(0.0), D(7.0), idx, d2, info, st)])
    wi, wd, winfo = sa.knn_descent(X, K, squared=True, n_projections=4, max_candidates=20, n_iters=3, delta=0.0, seed=7, ret_info=True)
    assert st[0] == 0
    same((idx, d2), (wi, wd))
    assert info.tolist() == [winfo["joins"], winfo["updates"], {"n_iters": 0, "delta": 1}[winfo["reason"]], winfo["gathered"]]
    assert 0 < winfo["gathered"] <= 3 * n * (40 * 40 + 40)
    L.sharp_C_knn_descent(*[P(v) for v in (X, D(n), I(10), I(600), I(4), I(20), I(3), D(0.0), D(7.0), idx, d2, info, st)])
    assert st[0] == 2 and "K must be in 1 .. 255" in L.sharp_last_error().decode()
