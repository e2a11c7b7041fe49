"""The Louvain specification (tests/_louvain_ref.py) on the CPU: the invariants the rules were designed for, the planted
partitions, the unit-weight path that a naive synchronous rule ruins, the quality on unstructured input against networkx, and the
package's refusals that need no device."""
import functools

import numpy as np
import pytest

import _louvain_ref as ref


@functools.lru_cache(maxsize=None)
def blobs():
    return ref.blobs_graph()


@functools.lru_cache(maxsize=None)
def blobs_run(gamma):
    rp, col, val = blobs()[:3]
    return ref.louvain(rp, col, val, gamma)


def nx_graph(rp, col, val):
    import networkx as nx

    row = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    up = row < col
    G = nx.Graph()
    G.add_nodes_from(range(len(rp) - 1))
    G.add_weighted_edges_from(zip(row[up].tolist(), col[up].tolist(), np.asarray(val, np.float64)[up].tolist()))
    return G


def nx_modularity(G, membership):
    import networkx as nx

    m = np.asarray(membership)
    return nx.community.modularity(G, [set(np.flatnonzero(m == c).tolist()) for c in np.unique(m)], weight="weight")


def nx_louvain_range(G, seeds=10):
    import networkx as nx

    qs = [nx.community.modularity(G, nx.community.louvain_communities(G, weight="weight", seed=s), weight="weight") for s in range(seeds)]
    return min(qs), max(qs)


# ---- invariants -----------------------------------------------------------------------------------------------------------------------
def test_accepted_rounds_never_lower_q():
    rp, col, val = blobs()[:3]
    rp, col, q = ref.drop_zeros(rp, col, ref.quantise(rp, col, val)[0])
    trace = []
    comm, rounds, Q = ref.level(rp, col, q, 1.0, 10, 0, trace=trace)
    kept = [t[2] for t in trace if t[1]]
    assert len(trace) == rounds and len(kept) > 10
    assert all(b > a for a, b in zip(kept, kept[1:])) and kept[-1] == Q
    assert Q == ref.state(rp, col, q, comm, 1.0)[3]
    assert not any(t[1] for t in trace[-ref.MAX_FAILS:]) or rounds == ref.MAX_ROUNDS


def test_aggregation_preserves_2m_and_q_exactly():
    rp, col, val = blobs()[:3]
    rp, col, q = ref.drop_zeros(rp, col, ref.quantise(rp, col, val)[0])
    for gamma in (1.0, 0.25):
        comm = ref.level(rp, col, q, gamma, 10, 0, max_rounds=30)[0]
        Q = ref.state(rp, col, q, comm, gamma)[3]
        crp, ccol, cq, new = ref.aggregate(rp, col, q, comm)
        nc = len(crp) - 1
        assert int(cq.sum()) == int(q.sum()) and nc == np.unique(comm).size
        assert ref.state(crp, ccol, cq, np.arange(nc), gamma)[3] == Q          # the same bits, not a close value
        row = np.repeat(np.arange(nc), np.diff(crp))
        assert (np.diff(row * nc + ccol) > 0).all() and (cq > 0).all()
        assert np.array_equal(ref.strengths(crp, cq), ref.state(rp, col, q, comm, gamma)[0][new >= 0])


def test_composed_labels_reproduce_every_levels_q():
    rp, col, val = blobs()[:3]
    r = blobs_run(1.0)
    for lev in r["levels"]:
        assert ref.modularity(rp, col, val, lev["membership"]) == lev["modularity"]
    assert ref.modularity(rp, col, val, r["membership"]) == r["modularity"]
    assert [lev["n"] for lev in r["levels"][1:]] == [lev["communities"] for lev in r["levels"][:-1]]
    assert r["levels"][-1]["communities"] == r["levels"][-1]["n"]               # the run ended at a level that merged nothing


def test_the_function_is_pure():
    rp, col, val = blobs()[:3]
    a, b = blobs_run(1.0), ref.louvain(rp.copy(), col.copy(), val.copy(), 1.0)
    assert np.array_equal(a["membership"], b["membership"])
    assert [(x["rounds"], x["modularity"]) for x in a["levels"]] == [(x["rounds"], x["modularity"]) for x in b["levels"]]


def test_fixed_sum_is_the_two_stage_order():
    rng = np.random.default_rng(0)
    for n in (1, 255, 256, 257, 1000, 300000):
        v = rng.normal(size=n)
        chunk = max(256, (n + 1023) // 1024)
        part = []
        for b0 in range(0, n, chunk):
            blk = v[b0:b0 + chunk]
            s = [0.0] * 256
            for t in range(min(256, blk.size)):
                for x in blk[t::256]:
                    s[t] = s[t] + x
            w = 128
            while w:
                for t in range(w):
                    s[t] = s[t] + s[t + w]
                w >>= 1
            part.append(s[0])
        s = [0.0] * 256
        for t in range(min(256, len(part))):
            for x in part[t::256]:
                s[t] = s[t] + x
        w = 128
        while w:
            for t in range(w):
                s[t] = s[t] + s[t + w]
            w >>= 1
        assert ref.fixed_sum(v) == s[0]
        assert abs(ref.fixed_sum(v) - v.sum()) <= 1e-9 * max(1.0, np.abs(v).sum())


def test_relabel_by_size():
    lab = np.array([7, 7, 3, 3, 9, 9, 9, 1])
    assert ref.relabel_by_size(lab).tolist() == [2, 2, 3, 3, 1, 1, 1, 4]         # ties (7 and 3): the smallest member first


# ---- planted partitions ---------------------------------------------------------------------------------------------------------------
def test_blobs_at_resolution_one_is_the_planted_partition():
    lab = blobs()[3]
    r = blobs_run(1.0)
    assert r["n_communities"] == 6 and ref.adjusted_rand(r["membership"], lab) == 1.0


def test_blobs_at_other_resolutions():
    """what this reference and networkx's louvain_communities (seeds 0 .. 9, checked when the test was written) both give: at 0.25 the
    planted partition still, at 4 a refinement of it -- more than six communities, none across two planted clusters"""
    lab = blobs()[3]
    low, high = blobs_run(0.25), blobs_run(4.0)
    assert ref.adjusted_rand(low["membership"], lab) == 1.0
    m = high["membership"]
    assert high["n_communities"] > 6
    assert all(np.unique(lab[m == c]).size == 1 for c in np.unique(m))


def test_twelve_blobs():
    import _umap_ref as U

    X, lab = U.blobs(3000, 10, 12, 0)
    r = ref.louvain(*ref.knn_graph(X, 14))
    assert r["n_communities"] == 12 and ref.adjusted_rand(r["membership"], lab) == 1.0


# ---- ties and quality against networkx ------------------------------------------------------------------------------------------------
def floor_of(lo, hi):
    """networkx's lowest Q over ten seeds minus three times its own highest-minus-lowest: the scale at which two runs of one heuristic
    disagree"""
    return lo - 3.0 * (hi - lo)


def test_unit_weight_path_is_not_ruined_by_ties():
    rp, col, val = ref.path(1025)
    r = ref.louvain(rp, col, val)
    G = nx_graph(rp, col, val)
    lo, hi = nx_louvain_range(G)
    q = nx_modularity(G, r["membership"])
    print(f"path: reference Q {r['modularity']:.6f} (networkx's formula {q:.6f}), networkx {lo:.6f} .. {hi:.6f}, floor {floor_of(lo, hi):.6f}")
    assert abs(q - r["modularity"]) < 1e-6                    # the quantised weights are all 2^24: the same graph
    assert q >= floor_of(lo, hi)


def test_quality_on_unstructured_input():
    rp, col, val = ref.gaussian_graph()[:3]
    r = ref.louvain(rp, col, val)
    G = nx_graph(rp, col, val)
    lo, hi = nx_louvain_range(G)
    q = nx_modularity(G, r["membership"])
    print(f"gaussian: reference Q {r['modularity']:.6f} (on the float weights {q:.6f}), networkx {lo:.6f} .. {hi:.6f}, "
          f"floor {floor_of(lo, hi):.6f}, communities {r['n_communities']}")
    assert abs(q - r["modularity"]) < 1e-6                    # quantisation moves a weight by 2^-25 of the largest at most
    assert q >= floor_of(lo, hi)


# ---- the package's refusals (no device) -----------------------------------------------------------------------------------------------
def test_python_side_refusals():
    import sharp_amd
    from sharp_amd import SharpError

    rp, col, val = ref.ring_of_cliques()
    n = len(rp) - 1

    def refused(match, fn, *a, **k):
        with pytest.raises(SharpError, match=match):
            fn(*a, **k)

    g = sharp_amd.louvain_graph
    bad = val.copy()
    bad[0] = 0.5
    refused("louvain_graph: the graph is not symmetric", g, rp, col, bad)
    keep = np.ones(col.size, bool)
    keep[0] = False                                           # one direction of an edge is missing
    rp2 = rp.copy()
    rp2[1:] -= 1
    refused("not symmetric", g, rp2, col[keep], val[keep])
    drp, dcol, dval = ref.csr_from_pairs(4, [0, 0, 1, 2], [0, 1, 2, 3], np.ones(4))
    refused("a diagonal entry", g, drp, dcol, dval)
    for v in (-1.0, np.nan, np.inf, 1e101):
        bad = val.copy()
        bad[2] = v
        refused("NA / NaN / Inf, negative or beyond 1e100", g, rp, col, bad)
    refused("no positive weight", g, rp, col, np.zeros_like(val))
    refused("holds no entry", g, np.zeros(5, np.int64), np.zeros(0, np.int32), np.zeros(0))
    refused("row_ptr must hold", g, rp[:-1], col, val)
    refused("column index out of range", g, rp, np.where(np.arange(col.size) == 1, n, col), val)
    refused("ascend strictly", g, rp, np.r_[col[1], col[0], col[2:]], val)
    for r in (0.0, -1.0, np.nan, np.inf, 2e6):
        refused("resolution must be in \\(0, 1e6\\]", g, rp, col, val, resolution=r)
    refused("tol must be finite", g, rp, col, val, tol=-1.0)
    refused("max_levels must be in 1 .. 64", g, rp, col, val, max_levels=0)
    refused("max_rounds must be in 1 .. 100000", g, rp, col, val, max_rounds=0)
    refused("max_fails must be in 1 .. 64", g, rp, col, val, max_fails=65)
    refused("seed must be a finite integer", g, rp, col, val, seed=1.5)
    refused("modularity: membership must hold n integer labels", sharp_amd.modularity, rp, col, val, np.zeros(n - 1, np.int64))
    refused("modularity: the graph is not symmetric", sharp_amd.modularity, rp2, col[keep], val[keep], np.zeros(n, np.int64))
    idx = (np.arange(40)[:, None] + np.arange(1, 4)[None, :]) % 40
    refused("louvain_neighbors: index .* differ in shape", sharp_amd.louvain_neighbors, idx, np.ones((40, 2)))
    refused("louvain_neighbors: resolution", sharp_amd.louvain_neighbors, idx, np.ones((40, 3)), resolution=0)
    X = np.zeros((30, 4))
    refused("louvain: n_neighbors must be in 2 .. 256", sharp_amd.louvain, X, n_neighbors=1)
    refused("louvain: n_neighbors must be smaller", sharp_amd.louvain, X, n_neighbors=30)
    refused("louvain: nn_args belong", sharp_amd.louvain, X, nn_args={"n_iters": 3})
    refused("louvain: nn_method", sharp_amd.louvain, X, nn_method="annoy")
    bad = X.copy()
    bad[3, 1] = np.nan
    refused("louvain: the input holds NA / NaN / Inf \\(row 4, column 2\\)", sharp_amd.louvain, bad)


def test_without_a_device_the_calls_fail_loudly(monkeypatch):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import sharp_amd

    monkeypatch.setattr(sharp_amd._lib, "_initialised_device", 0)
    rp, col, val = ref.ring_of_cliques()
    with pytest.raises(sharp_amd.SharpError, match="no device context|no HIP device"):
        sharp_amd.louvain_graph(rp, col, val)
    with pytest.raises(sharp_amd.SharpError, match="no device context|no HIP device"):
        sharp_amd.modularity(rp, col, val, np.zeros(len(rp) - 1, np.int64))
