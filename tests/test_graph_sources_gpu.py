"""The three graph sources behind louvain, leiden and diffmap (csrc/graph_source.hpp) on the MI355X: a method gives the
same bits whether its graph is built on the device from the caller's neighbour lists or handed over as the CSR of the same graph.
Every comparison is exact.  n = 300 rows of 8 columns with K = 10 is the smallest shape that still crosses the shared front with more
than one workgroup; the kernels behind it are tested at their own boundaries in their own files."""
import functools
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, K = 300, 8, 10
PRUNE = 1.0 / 15.0


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


@functools.lru_cache(maxsize=None)
def lists(squared):
    """(idx, d) of the rows of X = knn(X, K), or knn(X, K, squared=True)"""
    import sharp_amd

    X = np.random.default_rng(20261021).normal(size=(N, D))
    idx, d = sharp_amd.knn(X, K, squared=squared)
    idx.setflags(write=False)
    d.setflags(write=False)
    return idx, d


@functools.lru_cache(maxsize=None)
def fuzzy_csr():
    """(rp, col, val) of the lists' fuzzy graph, from the graph stage's wrapper (sharp_umap_graph)"""
    um = importlib.import_module("sharp_amd.umap")               # (sharp_amd.umap is the function)
    return um._graph(*lists(False))[:3]


def same_clustering(a, b):
    assert np.array_equal(a["membership"], b["membership"])
    assert np.float64(a["modularity"]).tobytes() == np.float64(b["modularity"]).tobytes()
    assert a["n_communities"] == b["n_communities"] and len(a["levels"]) == len(b["levels"])
    for la, lb in zip(a["levels"], b["levels"]):
        assert la.keys() == lb.keys()
        for key in la:
            if key == "membership":
                assert np.array_equal(la[key], lb[key])
            else:
                assert type(la[key]) is type(lb[key]) and np.array(la[key]).tobytes() == np.array(lb[key]).tobytes(), key


def same_map(a, b):
    assert np.array_equal(a["evals"], b["evals"])
    assert np.array_equal(a["evecs"], b["evecs"], equal_nan=True)
    assert np.array_equal(a["in_component"], b["in_component"])


@pytest.mark.parametrize("method", ["louvain", "leiden"])
@pytest.mark.parametrize("squared", [False, True])
def test_community_on_lists_is_community_on_their_fuzzy_graph(sa, method, squared):
    want = getattr(sa, method + "_graph")(*fuzzy_csr(), ret_levels=True)
    got = getattr(sa, method + "_neighbors")(*lists(squared), squared=squared, ret_levels=True)
    same_clustering(got, want)


@pytest.mark.parametrize("squared", [False, True])
def test_diffmap_on_lists_is_diffmap_on_their_fuzzy_graph(sa, squared):
    same_map(sa.diffmap_neighbors(*lists(squared), squared=squared), sa.diffmap_graph(*fuzzy_csr()))


@pytest.mark.parametrize("method", ["louvain", "leiden"])
def test_community_on_lists_is_community_on_their_snn_graph(sa, method):
    idx = lists(False)[0]
    g = sa.snn_graph(idx, PRUNE)
    want = getattr(sa, method + "_graph")(g["row_ptr"], g["col"], g["val"], ret_levels=True)
    same_clustering(getattr(sa, method + "_snn")(idx, PRUNE, ret_levels=True), want)


@pytest.mark.parametrize("method", ["louvain", "leiden"])
def test_a_prune_that_leaves_nothing_is_refused_by_name(sa, method):
    with pytest.raises(sa.SharpError, match=method + "_snn: the pruned graph holds no positive weight"):
        getattr(sa, method + "_snn")(lists(False)[0], 1.0)
