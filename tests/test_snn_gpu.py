"""The SNN / Jaccard graph on the MI355X against its numpy / scipy specification (tests/_snn_ref.py).  Every comparison is
exact: row_ptr, col, shared and the bytes of val.  The shapes are the smallest at which each part can go wrong: rows whose work t is
exactly the cap of each row class of the product kernels and one more, a table at its fullest (a ring: nearly all candidates of a row
distinct) and one with few keys that many lanes add to (the complete lists), rows of the dense class sharing a workgroup's counter row,
empty rows in the middle of the ids, n = 2, K = 1 and K = 255."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import _louvain_ref as lref
import _snn_ref as ref

pytestmark = pytest.mark.gpu

PRUNE = ref.PRUNE


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


def caps():
    return importlib.import_module("sharp_amd.snn")._row_caps()     # (sharp_amd.snn is the function)


def bits(x):
    return np.float64(x).tobytes()


def dense_lists(first_rows, second_rows=330, K=19):
    """K = 19: `first_rows` rows name one hub, `second_rows` further rows name 19 other hubs and nothing else; every one of them has more
    work than the workgroup class takes.  Returns (lists, the rows of both groups)."""
    n = 21 * (first_rows + second_rows) + 200
    lists = ref.ring(n, K)
    rows1 = 21 * np.arange(first_rows)
    rows2 = 21 * (first_rows + np.arange(second_rows))
    if first_rows:
        lists = ref.with_hub(lists, n - 1, rows1)
    for c in range(K):
        lists = ref.with_hub(lists, n - 2 - c, rows2, c)
    return lists, np.r_[rows1, rows2]


@functools.lru_cache(maxsize=None)
def case(name):
    """the lists of a case; computed once and left alone"""
    if name.startswith("blobs"):
        return ref.blobs_lists(int(name[5:]))[0]
    if name == "gaussian":
        return ref.gaussian_lists(19)[0]
    if name == "two":
        return np.array([[1], [0]], np.int32)
    if name.startswith("complete"):                          # every count is k: many lanes add to few keys
        return ref.complete_lists(int(name[8:]))
    if name == "n257":                                       # K = 255 of the 256 other rows: row i leaves out i + 1
        return np.array([[j for j in range(257) if j != i and j != (i + 1) % 257] for i in range(257)], np.int32)
    if name == "ring4099":
        return ref.ring(4099, 30)
    if name == "pair":
        return ref.isolated_pair_lists()
    if name.startswith("t"):
        return ref.boundary_case(int(name[1:]))[0]
    if name == "dense":
        return dense_lists(caps()[1] + 56)[0]
    if name == "dense_small":
        return dense_lists(0)[0]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def want(name, prune=PRUNE):
    return ref.snn_scipy(case(name), prune)


def check(sa, name, prune=PRUNE):
    got = sa.snn_graph(case(name), prune, ret_shared=True)
    ref.same_graph(got, want(name, prune))
    assert got["k"] == case(name).shape[1] + 1
    return got


# ---- the graph ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prune", [("blobs19", PRUNE), ("blobs9", PRUNE), ("gaussian", PRUNE), ("blobs1", PRUNE), ("blobs1", 0.0),
                                        ("two", PRUNE), ("complete256", PRUNE), ("complete32", PRUNE), ("complete40", 0.0), ("n257", PRUNE), ("ring4099", PRUNE), ("ring4099", 0.0),
                                        ("pair", 1.0), ("blobs9", 0.0), ("blobs9", 1.0)])
def test_graph_equals_the_reference(sa, name, prune):
    got = check(sa, name, prune)
    if name == "two":
        assert got["val"].tolist() == [1.0, 1.0] and got["shared"].tolist() == [2, 2]
    if name.startswith("complete"):                          # n = 32: t = 1024, the wave class; 40: the workgroup class; 256: the dense class
        m = case(name).shape[0]
        assert (got["shared"] == m).all() and got["nnz"] == m * (m - 1) and (ref.work(case(name)) == m * m).all()
    if name == "pair":
        assert got["col"].tolist() == [21, 20] and np.diff(got["row_ptr"])[:20].sum() == 0 and np.diff(got["row_ptr"])[22:].sum() == 0
    if name == "gaussian":                                   # the wave and the workgroup class are mixed
        w = ref.work(case(name))
        assert (w <= caps()[0]).any() and (w > caps()[0]).any() and w.max() <= caps()[1]


def test_every_row_class_boundary(sa):
    """rows with t exactly the cap of the wave class and of the workgroup class, and one more"""
    wave_cap, block_cap = caps()
    for t in (wave_cap, wave_cap + 1, block_cap, block_cap + 1):
        lists, rows = ref.boundary_case(t)
        assert (ref.work(lists)[rows] == t).all() and rows.size >= 100
        check(sa, f"t{t}")
    check(sa, f"t{wave_cap}", 0.0)                           # s = 1 too: every pair of the rows that share a hub


def test_dense_class(sa):
    """one hub named by more rows than the workgroup class takes, and 330 further rows of the dense class in the same launch: at most 128
    workgroups serve them, each on the counter row the row before it used and zeroed"""
    _, block_cap = caps()
    lists, rows = dense_lists(block_cap + 56)
    w = ref.work(lists)
    assert (w[rows] > block_cap).all() and rows.size > block_cap + 300 and rows.size > 2 * 128
    assert (np.bincount(lists.ravel())[-1] > block_cap)       # the hub's reverse neighbours
    got = check(sa, "dense")
    assert got["nnz"] < 10_000_000                           # the pruned form: megabytes


def test_dense_class_without_pruning(sa):
    """s = 1 and s = 2 out of the dense class (and s = 19: two rows that name the same 19 hubs)"""
    lists, rows = dense_lists(0)
    assert (ref.work(lists)[rows] > caps()[1]).all()
    got = check(sa, "dense_small", 0.0)
    rp, sh = got["row_ptr"], got["shared"]
    of_dense = np.concatenate([sh[rp[r]:rp[r + 1]] for r in rows])
    assert (of_dense == 1).any() and (of_dense == 2).any() and (of_dense == 19).any()


def test_the_tie_at_one_fifteenth(sa):
    assert 2.0 / 30.0 == 1.0 / 15.0
    got = check(sa, "blobs15")
    assert got["shared"].min() == 2 and (got["shared"] == 2).any()
    got = check(sa, "blobs19")
    assert got["shared"].min() == 3


def test_two_calls_give_the_same_bits(sa):
    for name, prune in (("gaussian", PRUNE), ("dense_small", 0.0)):
        a = sa.snn_graph(case(name), prune, ret_shared=True)
        b = sa.snn_graph(case(name), prune, ret_shared=True)
        for key in ("row_ptr", "col", "val", "shared"):
            assert a[key].tobytes() == b[key].tobytes()


def test_count_then_fill(sa):
    from sharp_amd._lib import f64, i32, i64, lib

    lists = case("blobs9")
    n, K = lists.shape
    rp, col, val, sh = want("blobs9")
    nnz = int(rp[-1])
    got_rp, got = np.zeros(n + 1, np.int64), C.c_longlong(-1)
    assert lib().sharp_snn_graph(i32(lists), n, K, PRUNE, 0, i64(got_rp), None, None, None, C.byref(got)) == 0
    assert got.value == nnz and np.array_equal(got_rp, rp)
    gc, gv, gs = np.zeros(nnz, np.int32), np.zeros(nnz), np.zeros(nnz, np.int32)
    got_rp[:] = 0
    assert lib().sharp_snn_graph(i32(lists), n, K, PRUNE, nnz, i64(got_rp), i32(gc), f64(gv), i32(gs), C.byref(got)) == 0
    assert got.value == nnz and np.array_equal(got_rp, rp) and np.array_equal(gc, col) and gv.tobytes() == val.tobytes()
    assert np.array_equal(gs, sh)
    gc[:] = -7
    got = C.c_longlong(-1)
    rc = lib().sharp_snn_graph(i32(lists), n, K, PRUNE, nnz - 1, i64(got_rp), i32(gc), f64(gv), None, C.byref(got))
    assert rc != 0 and got.value == nnz and str(nnz).encode() in lib().sharp_last_error() and b"cap" in lib().sharp_last_error()
    assert (gc == -7).all()                                  # nothing was filled


# ---- Louvain on it --------------------------------------------------------------------------------------------------------------------
def same_run(got, w):
    assert np.array_equal(got["membership"], w["membership"]) and got["n_communities"] == w["n_communities"]
    assert bits(got["modularity"]) == bits(w["modularity"]) and len(got["levels"]) == len(w["levels"])
    for g, l in zip(got["levels"], w["levels"]):
        assert (g["n"], g["communities"], g["rounds"]) == (l["n"], l["communities"], l["rounds"]) and bits(g["modularity"]) == bits(l["modularity"])


@functools.lru_cache(maxsize=None)
def ref_run(name, gamma):
    rp, col, val, _ = want(name)
    return lref.louvain(rp, col, val, gamma)


@pytest.mark.parametrize("name,gamma", [("blobs19", 1.0), ("blobs19", 0.25), ("blobs19", 4.0), ("dense_small", 1.0)])
def test_louvain_snn_equals_louvain_graph_and_the_reference(sa, name, gamma):
    lists = case(name)
    a = sa.louvain_snn(lists, resolution=gamma)
    g = sa.snn_graph(lists)
    b = sa.louvain_graph(g["row_ptr"], g["col"], g["val"], resolution=gamma)
    same_run(a, b)
    same_run(a, ref_run(name, gamma))
    if name == "blobs19" and gamma == 1.0:
        assert a["n_communities"] == 6 and lref.adjusted_rand(a["membership"], ref.blobs_lists(19)[1]) == 1.0
        lv = sa.louvain_snn(lists, ret_levels=True)
        assert np.array_equal(lv["levels"][-1]["membership"], sa.louvain_graph(g["row_ptr"], g["col"], g["val"], ret_levels=True)["levels"][-1]["membership"])


def test_front_doors(sa):
    X = ref.blobs_lists(19)[2]
    idx, dist = sa.knn(X, 19)
    a = sa.louvain(X, n_neighbors=20, graph="snn", ret_nn=True)
    assert np.array_equal(a["nn"]["index"], idx)
    same_run(a, sa.louvain_snn(idx))
    b = sa.louvain(X, n_neighbors=20, graph="snn", prune=0.2, resolution=0.5)
    same_run(b, sa.louvain_snn(idx, 0.2, resolution=0.5))
    # the default graph is the fuzzy one, unchanged
    nb = sa.knn(X, 14)
    f = sa.louvain_neighbors(*nb)
    same_run(sa.louvain(X), f)
    same_run(sa.louvain(X, graph="fuzzy"), f)
    # snn() is snn_graph() on knn()'s lists
    s = sa.snn(X, ret_nn=True)
    g = sa.snn_graph(idx)
    assert np.array_equal(s["nn"]["index"], idx) and s["k"] == 20
    for key in ("row_ptr", "col", "val"):
        assert s[key].tobytes() == g[key].tobytes()
    d = sa.snn(X, k_param=10, prune=0.0, nn_method="descent", ret_nn=True)
    di = sa.knn_descent(X, 9)[0]
    assert d["nn"]["method"] == "descent" and np.array_equal(d["nn"]["index"], di)
    gd = sa.snn_graph(di, 0.0)
    for key in ("row_ptr", "col", "val"):
        assert d[key].tobytes() == gd[key].tobytes()


def test_refusals_by_message(sa):
    lists = case("blobs9").copy()
    bad = lists.copy()
    bad[7, 2] = 1500
    with pytest.raises(sa.SharpError, match=r"snn_graph: a neighbour index outside \[0, n\) \(row 7, counted from 0\)"):
        sa.snn_graph(bad)
    bad[7, 2] = -1
    with pytest.raises(sa.SharpError, match=r"louvain_snn: a neighbour index outside \[0, n\) \(row 7"):
        sa.louvain_snn(bad)
    bad = lists.copy()
    bad[11, 0] = 11
    with pytest.raises(sa.SharpError, match=r"snn_graph: a row names itself as a neighbour \(row 11"):
        sa.snn_graph(bad)
    bad = lists.copy()
    bad[13, 8] = bad[13, 1]
    with pytest.raises(sa.SharpError, match=r"snn_graph: the same neighbour index twice in a row \(row 13"):
        sa.snn_graph(bad)
    with pytest.raises(sa.SharpError, match=r"louvain_snn: the same neighbour index twice in a row \(row 13"):
        sa.louvain_snn(bad)
    with pytest.raises(sa.SharpError, match=r"prune must be in \[0, 1\]"):
        sa.snn_graph(lists, 1.01)
    with pytest.raises(sa.SharpError, match="K <= n - 1"):
        sa.snn_graph(ref.ring(4, 3)[:3])
    with pytest.raises(sa.SharpError, match="louvain_snn: .*holds no positive weight"):
        sa.louvain_snn(ref.ring(64, 1), 1.0)                 # K = 1 ring: no two rows have equal sets
