"""The Leiden specification (tests/_leiden_ref.py) on the CPU: the invariants of the refinement and of the next level's
start on every case of _louvain_ref.py, the level-0 move phase against Louvain's, connected results, the planted partitions, a
community that is deliberately disconnected, the quality on unstructured input against networkx, and the package's refusals that need no
device.  Nothing here asserts that Leiden's Q is at least Louvain's: it is not always (DESIGN.md §25's table)."""
import functools

import numpy as np
import pytest
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

import _leiden_ref as ld
import _louvain_ref as ref
from test_louvain_cpu import floor_of, nx_graph, nx_louvain_range, nx_modularity


@functools.lru_cache(maxsize=None)
def case(name):
    """(rp, col, q) of an integer-weighted graph; computed once and left alone"""
    if name == "blobs":
        return ld.int_graph(*ref.blobs_graph()[:3])
    if name == "gaussian":
        return ld.int_graph(*ref.gaussian_graph()[:3])
    if name == "path":
        return ld.int_graph(*ref.path())
    if name == "ring":
        return ld.int_graph(*ref.ring_of_cliques())
    if name == "star":
        return ld.int_graph(*ref.star())
    if name == "planted":
        return ld.int_graph(*ref.planted()[:3])
    if name == "complete":
        return ref.complete_int(120)
    if name == "hub":
        return ref.hub(300)
    if name == "hubs":
        return ref.hubs(400, 5)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def run(name, gamma=1.0, seed=10):
    trace = []
    r = ld.leiden_q(*case(name), gamma, seed, check=False, trace=trace)
    return r, trace


def components_within(rp, col, label):
    """the number of connected pieces of every label's vertices, by scipy: (labels, pieces per label)"""
    rp, col, label = np.asarray(rp, np.int64), np.asarray(col, np.int64), np.asarray(label, np.int64)
    n = rp.size - 1
    row = np.repeat(np.arange(n), np.diff(rp))
    keep = label[row] == label[col]
    A = csr_matrix((np.ones(int(keep.sum())), (row[keep], col[keep])), shape=(n, n))
    comp = connected_components(A, directed=False)[1]
    pairs = np.unique(np.stack([label, comp]), axis=1)
    return np.unique(pairs[0], return_counts=True)


ALL = ["blobs", "gaussian", "path", "ring", "star", "planted", "complete", "hub", "hubs"]


# ---- invariants -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_refinement_invariants(name):
    r, trace = run(name)
    assert len(trace) == len(r["levels"])
    for lev, t in zip(r["levels"], trace):
        rp, col, q = t["graph"]
        P, sub = np.asarray(t["P"], np.int64), np.asarray(t["ref"], np.int64)
        n = len(rp) - 1
        # inside P: a sub-community's members share one community
        assert np.unique(sub * n + P).size == np.unique(sub).size == lev["sub_communities"]
        # connected in the level's graph
        assert (components_within(rp, col, sub)[1] == 1).all()
        # the next start: every community connected
        if t["comm0"] is not None:
            assert (components_within(rp, col, t["comm0"])[1] == 1).all()
        # a sub-community that gains in a round loses nothing in it, and only singletons move
        assert len(t["rounds"]) == lev["refine_rounds"]
        for before, after in t["rounds"]:
            before, after = np.asarray(before), np.asarray(after)
            moved = before != after
            assert not np.isin(before[moved], after[moved]).any()
            assert (np.bincount(before, minlength=n)[before[moved]] == 1).all()
    assert [lev["n"] for lev in r["levels"][1:]] == [lev["sub_communities"] for lev in r["levels"][:-1]]
    last = r["levels"][-1]
    assert last["sub_communities"] == last["n"]               # the run ended at a level whose refinement merged nothing


def test_the_reference_asserts_its_invariants_itself():
    """check=True (the default) runs the reference's own assertions on the same cases"""
    r = ld.leiden_q(*case("blobs"))
    assert np.array_equal(r["membership"], run("blobs")[0]["membership"])
    rp, col, q = case("ring")
    P = np.arange(len(rp) - 1) // 6 * 6
    bad = np.zeros(len(rp) - 1, np.int64)                     # one sub-community over every clique: across communities
    with pytest.raises(AssertionError, match="across two communities"):
        ld.check_refinement(rp, col, P, bad)
    with pytest.raises(AssertionError, match="not connected"):
        v = np.arange(bad.size)                               # the first and the third clique as one sub-community: they do not touch
        ld.check_refinement(rp, col, np.zeros_like(bad), np.where((v < 6) | ((v >= 12) & (v < 18)), 0, v))


def test_level_zero_is_louvains_level():
    for name, gamma in (("blobs", 1.0), ("path", 1.0), ("planted", 4.0)):
        rp, col, q = case(name)
        a = ld.level(rp, col, q, gamma, 10, 0)
        b = ref.level(rp, col, q, gamma, 10, 0)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.float64(a[2]).tobytes() == np.float64(b[2]).tobytes()
        lev0 = ld.leiden_q(rp, col, q, gamma, max_levels=1)["levels"][0]
        assert (lev0["rounds"], lev0["communities"]) == (b[1], np.unique(b[0]).size) and lev0["modularity"] == b[2]


@pytest.mark.parametrize("name,gamma", [(n, 1.0) for n in ALL] + [("blobs", 4.0), ("gaussian", 4.0), ("planted", 3.0)])
def test_returned_communities_are_connected_and_q_is_modularity_q(name, gamma):
    r = run(name, gamma)[0]
    rp, col, q = case(name)
    labels, pieces = components_within(rp, col, r["membership"])
    assert labels.size == r["n_communities"] and (pieces == 1).all()
    assert np.float64(r["modularity"]).tobytes() == np.float64(ref.modularity_q(rp, col, q, r["membership"], gamma)).tobytes()
    sizes = np.bincount(r["membership"])[1:]
    assert r["membership"].min() == 1 and (np.diff(sizes) <= 0).all()


def test_the_function_is_pure():
    rp, col, q = case("gaussian")
    a, b = run("gaussian")[0], ld.leiden_q(rp.copy(), col.copy(), q.copy())
    assert np.array_equal(a["membership"], b["membership"]) and a["modularity"] == b["modularity"]
    key = lambda r: [(x["rounds"], x["refine_rounds"], x["sub_communities"], x["modularity"]) for x in r["levels"]]   # noqa: E731
    assert key(a) == key(b)


# ---- planted partitions ---------------------------------------------------------------------------------------------------------------
def test_planted_partitions_are_recovered():
    lab = ref.blobs_graph()[3]
    for gamma in (1.0, 0.25):
        r = run("blobs", gamma)[0]
        assert r["n_communities"] == 6 and ref.adjusted_rand(r["membership"], lab) == 1.0
    # the noisy planted partition: a vertex whose weight towards another block exceeds that towards its own (vertex 134 of this graph)
    # is planted on the wrong side of the noise; everywhere else the blocks are found, and Q is no lower than the planted labelling's
    rp, col, q = case("planted")
    lab = ref.planted()[3]
    row = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    w = np.zeros((len(lab), 8), np.int64)
    np.add.at(w, (row, lab[col]), q)
    clear = w.argmax(1) == lab
    r = run("planted")[0]
    assert r["n_communities"] == 8 and clear.sum() >= len(lab) - 2
    assert ref.adjusted_rand(r["membership"][clear], lab[clear]) == 1.0
    assert r["modularity"] >= ref.modularity_q(rp, col, q, lab)
    r = run("ring")[0]
    assert r["n_communities"] == 30 and ref.adjusted_rand(r["membership"], np.arange(180) // 6) == 1.0


# ---- a community that is not connected ------------------------------------------------------------------------------------------------
def test_a_disconnected_community_is_never_bridged_and_is_split():
    rp, col, q, P = ld.cliques_across_a_gap()
    assert components_within(rp, col, P)[1].tolist() == [2, 1]           # the first community is in two pieces
    sub, rounds = ld.refine(rp, col, q, P, 1.0, 10, 0)
    assert rounds > 0 and np.unique(sub).size < len(P)
    assert not np.isin(sub[:6], sub[6:12]).any()                          # no sub-community across the gap
    assert (components_within(rp, col, sub)[1] == 1).all()
    # L3: the next level starts from the connected parts of the parents
    crp, ccol, cq, new = ref.aggregate(rp, col, q, sub)
    parent = np.zeros(len(crp) - 1, np.int64)
    parent[new[sub]] = P
    comm0 = ld.split(crp, ccol, parent)
    left, right = np.unique(comm0[new[sub[:6]]]), np.unique(comm0[new[sub[6:12]]])
    assert left.size == 1 and right.size == 1 and left[0] != right[0]
    assert (components_within(crp, ccol, comm0)[1] == 1).all()
    # L4: the returned partition is split the same way
    out = ld.split(rp, col, P)
    assert out.tolist() == [0] * 6 + [6] * 6 + [12] * 2
    # the split never lowers Q for gamma > 0
    for gamma in (1.0, 0.25, 4.0):
        assert ref.modularity_q(rp, col, q, out, gamma) >= ref.modularity_q(rp, col, q, P, gamma)


def test_split_ignores_self_loops_and_names_components_by_their_smallest_vertex():
    rp, col, q = ref.csr_from_pairs(5, [0, 1, 2, 3, 4, 1], [0, 1, 2, 3, 4, 3], np.ones(6, np.int64))
    assert ld.split(rp, col, np.zeros(5)).tolist() == [0, 1, 2, 1, 4]
    assert ld.split(rp, col, np.array([0, 0, 0, 1, 1])).tolist() == [0, 1, 2, 3, 4]


# ---- quality against networkx ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gaussian", "path"])
def test_quality_floor(name):
    """Q >= networkx's lowest Louvain Q of ten seeds minus three times its spread, computed here (test_louvain_cpu.py's floor)"""
    rp, col, val = ref.gaussian_graph()[:3] if name == "gaussian" else ref.path(1025)
    r = ld.leiden(rp, col, val)
    G = nx_graph(rp, col, val)
    lo, hi = nx_louvain_range(G)
    q = nx_modularity(G, r["membership"])
    print(f"{name}: reference Leiden Q {r['modularity']:.6f} (networkx's formula on the float weights {q:.6f}), networkx Louvain "
          f"{lo:.6f} .. {hi:.6f}, floor {floor_of(lo, hi):.6f}, communities {r['n_communities']}")
    assert abs(q - r["modularity"]) < 1e-6
    assert q >= floor_of(lo, hi)


# ---- the package's refusals (no device) -----------------------------------------------------------------------------------------------
def test_python_side_refusals():
    import sharp_amd
    from sharp_amd import SharpError

    rp, col, val = ref.ring_of_cliques()

    def refused(match, fn, *a, **k):
        with pytest.raises(SharpError, match=match):
            fn(*a, **k)

    g = sharp_amd.leiden_graph
    bad = val.copy()
    bad[0] = 0.5
    refused("leiden_graph: the graph is not symmetric", g, rp, col, bad)
    drp, dcol, dval = ref.csr_from_pairs(4, [0, 0, 1, 2], [0, 1, 2, 3], np.ones(4))
    refused("leiden_graph: a diagonal entry", g, drp, dcol, dval)
    for v in (-1.0, np.nan, np.inf, 1e101):
        bad = val.copy()
        bad[2] = v
        refused("NA / NaN / Inf, negative or beyond 1e100", g, rp, col, bad)
    refused("no positive weight", g, rp, col, np.zeros_like(val))
    refused("holds no entry", g, np.zeros(5, np.int64), np.zeros(0, np.int32), np.zeros(0))
    refused("row_ptr must hold", g, rp[:-1], col, val)
    refused("ascend strictly", g, rp, np.r_[col[1], col[0], col[2:]], val)
    for r in (0.0, -1.0, np.nan, np.inf, 2e6):
        refused("leiden_graph: resolution must be in \\(0, 1e6\\]", g, rp, col, val, resolution=r)
    refused("tol must be finite", g, rp, col, val, tol=-1.0)
    refused("max_levels must be in 1 .. 64", g, rp, col, val, max_levels=0)
    refused("max_rounds must be in 1 .. 100000", g, rp, col, val, max_rounds=100001)
    refused("max_fails must be in 1 .. 64", g, rp, col, val, max_fails=65)
    refused("seed must be a finite integer", g, rp, col, val, seed=1.5)
    for m in (0, -3, 100001):
        refused("leiden_graph: max_refine_rounds must be in 1 .. 100000", g, rp, col, val, max_refine_rounds=m)
    idx = (np.arange(40)[:, None] + np.arange(1, 4)[None, :]) % 40
    refused("leiden_neighbors: index .* differ in shape", sharp_amd.leiden_neighbors, idx, np.ones((40, 2)))
    refused("leiden_neighbors: max_refine_rounds", sharp_amd.leiden_neighbors, idx, np.ones((40, 3)), max_refine_rounds=0)
    refused("leiden_snn: max_refine_rounds", sharp_amd.leiden_snn, idx, max_refine_rounds=0)
    refused("leiden_snn: resolution", sharp_amd.leiden_snn, idx, resolution=0)
    X = np.zeros((30, 4))
    refused("leiden: n_neighbors must be in 2 .. 256", sharp_amd.leiden, X, n_neighbors=1)
    refused("leiden: nn_args belong", sharp_amd.leiden, X, nn_args={"n_iters": 3})
    refused("leiden: graph must be", sharp_amd.leiden, X, graph="knn")
    refused("leiden: prune belongs", sharp_amd.leiden, X, prune=0.1)
    refused("leiden: max_refine_rounds", sharp_amd.leiden, X, max_refine_rounds=0)


def test_without_a_device_the_calls_fail_loudly(monkeypatch):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import sharp_amd

    monkeypatch.setattr(sharp_amd._lib, "_initialised_device", 0)
    rp, col, val = ref.ring_of_cliques()
    with pytest.raises(sharp_amd.SharpError, match="no device context|no HIP device"):
        sharp_amd.leiden_graph(rp, col, val)
