"""What every entry that takes neighbour lists says when the lists are spoiled (csrc/knn.hpp: one set of fault kinds, one decoder).
The lists are knn()'s of a seeded 40 x 3 Gaussian with K = 4 (tests/test_tsne_cpu.py pins that they are sound), spoiled one way at a
time in rows 7 and 23 at once: the lower row is the one reported.  The whole message is compared: the entry's own name, one of the
four texts, the row.  The texts are the library's from before the decoder was shared; only sharp_knn_descent_join's prefix is new (it
said Rtsne_neighbors).

umap_transform's stage entry for given lists (sharp_umap_transform_weights) checks on the host and in its own words: an index outside
the reference is named with its row, a bad distance without one, and a query row is no reference row, so "itself" and "twice" are not
faults there.  Its texts are pinned as they are.

umap(X) and louvain(X) reach the self search; with the input scaled by 1e200 the row norms overflow and the search refuses in the
caller's name (louvain(X) searches through knn(), which is Rtsne's stage and says so)."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, K, ROWS = 40, 3, 4, (7, 23)

RANGE = "a neighbour index outside [0, n)"
SELF = "a row names itself as a neighbour"
TWICE = "the same neighbour index twice in a row"
DIST = "a distance that is NA / NaN / Inf or negative"
SPOILINGS = {"index n": RANGE, "index -1": RANGE, "self": SELF, "twice": TWICE, "NaN distance": DIST, "negative distance": DIST}
ROW = " (row 7, counted from 0)"

# entry -> (the name its refusals begin with, whether it takes distances)
ENTRIES = {
    "Rtsne_neighbors": ("Rtsne_neighbors", True),
    "umap_neighbors": ("umap_neighbors", True),
    "louvain_neighbors": ("louvain_neighbors", True),
    "snn_graph": ("snn_graph", False),
    "louvain_snn": ("louvain_snn", False),
    "neighbor_ranks": ("sharp_neighbor_ranks", False),
    "knn_descent_join": ("sharp_knn_descent_join", False),
}


def gaussian():
    return np.random.default_rng(20261019).standard_normal((N, D))


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


@pytest.fixture(scope="module")
def lists(sa):
    X = gaussian()
    idx, dist = sa.knn(X, K)
    idx.setflags(write=False)
    dist.setflags(write=False)
    return X, idx, dist


def spoil(idx, dist, how):
    idx, dist = idx.copy(), dist.copy()
    for r in ROWS:
        if how == "index n":
            idx[r, 1] = N
        elif how == "index -1":
            idx[r, 1] = -1
        elif how == "self":
            idx[r, 2] = r
        elif how == "twice":
            idx[r, 3] = idx[r, 0]
        elif how == "NaN distance":
            dist[r, 1] = np.nan
        else:
            dist[r, 1] = -1.0
    return idx, dist


def call(sa, entry, X, idx, dist):
    from sharp_amd import tsne

    if entry == "Rtsne_neighbors":
        return sa.Rtsne_neighbors(idx, dist, perplexity=1, max_iter=0)
    if entry == "umap_neighbors":
        return sa.umap_neighbors(idx, dist, n_epochs=0)
    if entry == "louvain_neighbors":
        return sa.louvain_neighbors(idx, dist)
    if entry == "snn_graph":
        return sa.snn_graph(idx)
    if entry == "louvain_snn":
        return sa.louvain_snn(idx)
    if entry == "neighbor_ranks":
        return sa.neighbor_ranks(X, idx)
    return tsne._knn_descent_join(X, idx)


# (a spoiled distance is no case of an entry that takes no distances)
CASES = [(entry, how) for entry, (_, takes_distance) in ENTRIES.items() for how, text in SPOILINGS.items() if takes_distance or text != DIST]


@pytest.mark.parametrize("entry,how", CASES)
def test_spoiled_lists_are_refused_in_the_entrys_name(sa, lists, entry, how):
    prefix = ENTRIES[entry][0]
    X, idx, dist = lists
    call(sa, entry, X, idx, dist)                                                    # the unspoiled lists pass
    bad_idx, bad_dist = spoil(idx, dist, how)
    with pytest.raises(sa.SharpError) as e:
        call(sa, entry, X, bad_idx, bad_dist)
    assert str(e.value) == prefix + ": " + SPOILINGS[how] + ROW


@pytest.mark.parametrize("how", ["index n", "index -1", "NaN distance", "negative distance"])
def test_transform_stage_refuses_in_its_own_words(sa, lists, how):
    um = importlib.import_module("sharp_amd.umap")                                   # (sharp_amd.umap is the function)
    X, idx, dist = lists
    with sa.UmapModel(X, X[:, :2], K, 1.0, 1.0, 0) as model:
        um._transform_weights(model, idx, dist)
        bad_idx, bad_dist = spoil(idx, dist, how)
        with pytest.raises(sa.SharpError) as e:
            um._transform_weights(model, bad_idx, bad_dist)
    if SPOILINGS[how] == RANGE:
        assert str(e.value) == "sharp_umap_transform_weights: idx holds an index outside the reference (row 7)"
    else:
        assert str(e.value) == "sharp_umap_transform_weights: dist holds a value that is NA / NaN / Inf or negative"


OVERFLOW = "the (prepared) input holds NA / NaN / Inf, or values so large that squared distances overflow"


def test_self_search_refuses_overflowing_norms_in_the_callers_name(sa):
    X = gaussian() * 1e200
    with pytest.raises(sa.SharpError) as e:
        sa.umap(X, n_epochs=0)
    assert str(e.value) == "umap: " + OVERFLOW
    with pytest.raises(sa.SharpError) as e:
        sa.louvain(X)
    assert str(e.value) == "Rtsne: " + OVERFLOW
