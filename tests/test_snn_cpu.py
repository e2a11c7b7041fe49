"""The SNN / Jaccard graph specification (tests/_snn_ref.py) on the CPU: the two statements of it against each other, its
invariants, the tie at prune = 1/15, the quality of Louvain on it, the premises of the GPU tests' boundary cases (read from the library's
own caps, which need no device), and the package's refusals that need no device."""
import functools

import numpy as np
import pytest

import _louvain_ref as lref
import _snn_ref as ref


def same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes() and np.array_equal(a[3], b[3])


def small_hub_case():
    lists, rows = ref.hub_rows(400, 5, 2, 12)
    return lists


@functools.lru_cache(maxsize=None)
def blobs_ref(K, prune=ref.PRUNE):
    return ref.snn_scipy(ref.blobs_lists(K)[0], prune)


@pytest.mark.parametrize("name", ["blobs9", "ring", "hub", "two"])
def test_the_two_statements_agree(name):
    lists = {"blobs9": lambda: ref.blobs_lists(9)[0], "ring": lambda: ref.ring(301, 7), "hub": small_hub_case,
             "two": lambda: np.array([[1], [0]], np.int32)}[name]()
    for prune in (ref.PRUNE, 0.0):
        a, b = ref.snn_scipy(lists, prune), ref.snn_loop(lists, prune)
        same(a, b)
    if name == "two":
        assert a[0].tolist() == [0, 1, 2] and a[1].tolist() == [1, 0] and a[2].tolist() == [1.0, 1.0] and a[3].tolist() == [2, 2]
    if name == "ring":
        assert (ref.work(lists) == 64).all()                    # every in-degree is k, t = k^2


def test_invariants():
    for lists in (ref.blobs_lists(19)[0], small_hub_case()):
        rp, col, val, sh = ref.snn_scipy(lists, 0.0)
        n = rp.size - 1
        row = np.repeat(np.arange(n), np.diff(rp))
        assert (col != row).all()                                # no diagonal
        key = row * n + col
        assert (np.diff(key) > 0).all()                          # strictly ascending columns within a row
        at = np.searchsorted(key, col.astype(np.int64) * n + row)
        assert np.array_equal(key[at], col.astype(np.int64) * n + row)
        assert val[at].tobytes() == val.tobytes() and np.array_equal(sh[at], sh)      # symmetric bit for bit
        k = lists.shape[1] + 1
        assert sh.min() >= 1 and sh.max() <= k and (val == sh / (2.0 * k - sh)).all()


def test_the_tie_at_one_fifteenth():
    """K = 15: w(2) = 2 / 30 is the double 1 / 15, and Seurat zeroes value < prune only, so s = 2 stays.  K = 19 drops s = 2 and keeps s = 3."""
    assert 2.0 / 30.0 == 1.0 / 15.0
    sh = blobs_ref(15)[3]
    assert sh.min() == 2 and (sh == 2).sum() > 0
    assert (ref.snn_scipy(ref.blobs_lists(15)[0], 0.0)[3] == 1).sum() > 0
    sh = blobs_ref(19)[3]
    assert 2.0 / 38.0 < 1.0 / 15.0 <= 3.0 / 37.0
    assert sh.min() == 3 and (sh == 3).sum() > 0


def test_prune_zero_and_one():
    lists = ref.blobs_lists(9)[0]
    every = ref.snn_scipy(lists, 0.0)
    assert every[3].min() == 1
    assert every[0][-1] > blobs_ref(9)[0][-1]
    pair = ref.isolated_pair_lists()
    only = ref.snn_scipy(pair, 1.0)
    assert only[1].tolist() == [21, 20] and only[3].tolist() == [2, 2] and only[2].tolist() == [1.0, 1.0]
    assert np.diff(only[0])[:20].sum() == 0 and np.diff(only[0])[22:].sum() == 0     # empty rows on both sides of the pair
    assert (ref.snn_scipy(ref.complete_lists(12), 1.0)[3] == 12).all()


@pytest.mark.parametrize("K", [19, 9])
def test_louvain_on_the_snn_graph_finds_the_blobs(K):
    rp, col, val, _ = blobs_ref(K)
    r = lref.louvain(rp, col, val)
    assert r["n_communities"] == 6
    assert lref.adjusted_rand(r["membership"], ref.blobs_lists(K)[1]) == 1.0
    assert r["modularity"] > 0.83


def test_premises_of_the_gpu_boundary_cases():
    """the GPU file's boundary cases hold rows with t exactly equal to each cap of the product kernels and to each cap + 1"""
    import importlib

    wave_cap, block_cap = importlib.import_module("sharp_amd.snn")._row_caps()     # (sharp_amd.snn is the function)
    assert 256 < wave_cap < block_cap
    for t in (wave_cap, wave_cap + 1, block_cap, block_cap + 1):
        lists, rows = ref.boundary_case(t)
        w = ref.work(lists)
        assert (w[rows] == t).all() and rows.size >= 100
    # the measured rows the caps were chosen for: the blobs fit the wave class, the Gaussian case mixes the wave and the workgroup class
    wb = ref.work(ref.blobs_lists(19)[0])
    assert wb.min() == 334 and wb.max() == 969 and wb.max() <= wave_cap
    wg = ref.work(ref.gaussian_lists(19)[0])
    assert (wg <= wave_cap).any() and (wg > wave_cap).any() and wg.max() == 2362 and wg.max() <= block_cap


def test_refusals_that_need_no_device():
    import sharp_amd as sa

    lists = ref.ring(40, 3)
    for prune in (-0.1, 1.5, float("nan")):
        with pytest.raises(sa.SharpError, match=r"snn_graph: prune must be in \[0, 1\]"):
            sa.snn_graph(lists, prune)
        with pytest.raises(sa.SharpError, match=r"louvain_snn: prune must be in \[0, 1\]"):
            sa.louvain_snn(lists, prune)
    with pytest.raises(sa.SharpError, match="snn_graph: index must be an n x K matrix"):
        sa.snn_graph(lists.ravel())
    with pytest.raises(sa.SharpError, match="snn_graph: index must hold integers"):
        sa.snn_graph(lists.astype(np.float64))
    with pytest.raises(sa.SharpError, match="snn_graph: need 1 <= K <= 255 neighbours per row and K <= n - 1"):
        sa.snn_graph(ref.ring(4, 3)[:3])
    with pytest.raises(sa.SharpError, match="need 1 <= K <= 255"):
        sa.snn_graph(np.zeros((300, 256), np.int32))
    with pytest.raises(sa.SharpError, match="need 2 <= n"):
        sa.snn_graph(np.zeros((1, 1), np.int32))
    X = np.random.default_rng(0).normal(size=(50, 4))
    with pytest.raises(sa.SharpError, match="louvain: prune belongs to graph = \"snn\""):
        sa.louvain(X, prune=0.1)
    with pytest.raises(sa.SharpError, match="louvain: prune belongs to graph = \"snn\""):
        sa.louvain(X, graph="fuzzy", prune=1.0 / 15.0)
    with pytest.raises(sa.SharpError, match="louvain: graph must be"):
        sa.louvain(X, graph="jaccard")
    with pytest.raises(sa.SharpError, match=r"louvain: prune must be in \[0, 1\]"):
        sa.louvain(X, graph="snn", prune=2.0)
    with pytest.raises(sa.SharpError, match="snn: k_param must be in 2 .. 256"):
        sa.snn(X, k_param=1)
    with pytest.raises(sa.SharpError, match="snn: k_param must be smaller than the number of rows"):
        sa.snn(X, k_param=50)
    with pytest.raises(sa.SharpError, match=r"snn: prune must be in \[0, 1\]"):
        sa.snn(X, prune=-1.0)


def test_the_library_refuses_again_without_the_package():
    """what reaches the library without the package's checks is refused by name before any device work"""
    import ctypes as C

    from sharp_amd._lib import i32, i64, lib

    lists = ref.ring(40, 3)
    rp, nnz = np.zeros(41, np.int64), C.c_longlong(-1)
    for n, K, prune, msg in ((40, 3, 1.5, b"snn_graph: prune must be in [0, 1]"), (40, 3, float("nan"), b"prune must be in [0, 1]"),
                             (40, 0, 0.1, b"need 1 <= K <= 255"), (3, 3, 0.1, b"K <= n - 1"), (1, 1, 0.1, b"need 2 <= n")):
        rc = lib().sharp_snn_graph(i32(lists), n, K, prune, 0, i64(rp), None, None, None, C.byref(nnz))
        assert rc != 0 and msg in lib().sharp_last_error()
