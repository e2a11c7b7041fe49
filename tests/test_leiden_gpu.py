"""Leiden on the MI355X against the numpy specification (tests/_leiden_ref.py), stage by stage and end to end.  Every
comparison is exact: integers, or the bits of doubles.  The shapes are the smallest at which each part can go wrong: rows of exactly
the longest length of each row class of the refine kernel and one more, a hub whose candidates all tie, more dense-class rows than
workgroups that own a dense row, rows without an entry inside their community, an empty row, n = 2, and resolutions at which the
well-connectedness rules bite."""
import functools

import numpy as np
import pytest

import _leiden_ref as ld
import _louvain_ref as ref
from test_louvain_gpu import float_case, int_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


def bits(x):
    return np.float64(x).tobytes()


@functools.lru_cache(maxsize=None)
def graph(name):
    """(rp, col, q) of a level's graph"""
    if name == "planted":
        return ld.int_graph(*float_case("planted"))
    return int_case(name)


@functools.lru_cache(maxsize=None)
def move_phase(name, gamma=1.0):
    """the reference's P of the graph's level 0"""
    return ld.level(*graph(name), gamma, 10, 0)[0]


@functools.lru_cache(maxsize=None)
def ref_refinement(name, gamma=1.0, partition="move"):
    """(P, the states the reference's rounds start from and its end state)"""
    rp, col, q = graph(name)
    n = len(rp) - 1
    P = {"move": lambda: move_phase(name, gamma), "one": lambda: np.zeros(n, np.int32), "singletons": lambda: np.arange(n, dtype=np.int32)}[partition]()
    trace = []
    end, rounds = ld.refine(rp, col, q, P, gamma, 10, 0, trace=trace)
    return P, [t[0] for t in trace] + [end]


@functools.lru_cache(maxsize=None)
def ref_run(name, gamma, **kw):
    return ld.leiden(*float_case(name), gamma, **kw)


# ---- one refinement round -------------------------------------------------------------------------------------------------------------
def check_round(community, g, P, state, gamma=1.0, level=0, rnd=0, seed=10):
    got = community._leiden_refine(*g, P, state, gamma, seed, level, rnd)
    want = ld.refine_round(*g, P, state, gamma, seed, level, rnd)
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0])
    assert (got[1], got[2]) == (want[1], want[2])
    assert got[1] == int((got[0] != state).sum())
    return got[1], got[2]


def check_states(community, name, gamma=1.0, partition="move"):
    """the rounds from the singletons, after 1 and 3 reference rounds, the last counted round and the state after all of them (where
    nothing is left to want); every round of a refinement of fewer than eight"""
    g = graph(name)
    P, states = ref_refinement(name, gamma, partition)
    total = 0
    last = len(states) - 1
    for r in range(last + 1) if last < 8 else (0, 1, 3, last - 1, last):
        if True:
            moved, wanting = check_round(community, g, P, states[r], gamma, rnd=r)
            total += moved
            assert (wanting == 0) == (r == len(states) - 1 and len(states) - 1 < ld.MAX_REFINE_ROUNDS)
    return total, len(states) - 1


@pytest.mark.parametrize("name", ["blobs", "path", "ring", "complete", "two", "n257", "empty_row"])
def test_refine_inside_the_move_phases_partition(sa, name):
    from sharp_amd import community

    moved, rounds = check_states(community, name)
    if name not in ("complete", "two"):                      # (their move phases may end in the singletons, where nothing moves)
        assert moved > 0 and rounds > 0


@pytest.mark.parametrize("name", ["blobs", "complete", "n257", "two"])
def test_refine_inside_one_community(sa, name):
    from sharp_amd import community

    moved, rounds = check_states(community, name, partition="one")
    assert moved > 0 and rounds > 0


@pytest.mark.parametrize("name", ["blobs", "n257"])
def test_refine_inside_singletons_ends_at_once(sa, name):
    """every entry leads out of the vertex's community: nothing eligible has a candidate, wanting = 0"""
    from sharp_amd import community

    g = graph(name)
    n = len(g[0]) - 1
    v = np.arange(n, dtype=np.int32)
    assert check_round(community, g, v, v) == (0, 0)
    assert ref_refinement(name, 1.0, "singletons")[1][-1].tolist() == v.tolist()


def test_refine_other_levels_seeds_and_resolutions(sa):
    from sharp_amd import community

    g = graph("blobs")
    P, states = ref_refinement("blobs")
    for gamma, level, rnd, seed in ((0.25, 1, 2, 10), (4.0, 2, 7, 3), (1.0, 5, 99999, -8)):
        check_round(community, g, P, states[2], gamma, level, rnd, seed)


def test_refine_at_every_row_class_boundary(sa):
    """a row of exactly the longest length of the wave class and of the workgroup class, and one entry more, every entry inside the
    row's community: from the singletons (as many keys as entries) and after a round; and the same rows with a community that ends
    behind the boundary, so that the table holds fewer keys than the row has entries"""
    from sharp_amd import community

    wave_cap, block_cap = community._row_caps()
    for length in (wave_cap, wave_cap + 1, block_cap, block_cap + 1):
        g = graph(f"hub{length}")
        n = len(g[0]) - 1
        assert g[0][1] - g[0][0] == length
        one = np.zeros(n, np.int32)
        cut = np.where(np.arange(n) <= length - 7, 0, 1).astype(np.int32)       # the hub's last seven neighbours lie outside its community
        for P in (one, cut):
            v = np.arange(n, dtype=np.int32)
            moved = 0
            for rnd in range(4):                             # (the hub's source bit is open in about half the rounds)
                moved += check_round(community, g, P, v, rnd=rnd)[0]
            assert moved > 0
            nxt = ld.refine_round(*g, P, v, 1.0, 10, 0, 0)[0]
            check_round(community, g, P, nxt, rnd=1)


def test_refine_a_hub_whose_candidates_all_tie(sa):
    """a star of 3 100 leaves in one community (the dense class): every leaf is a candidate of the hub with the same gain, and the hub
    goes to the lowest id whose bit allows it"""
    from sharp_amd import community

    _, block_cap = community._row_caps()
    g = ld.int_graph(*float_case("star3100"))
    n = len(g[0]) - 1
    assert g[0][1] - g[0][0] == 3100 > block_cap
    P, v = np.zeros(n, np.int32), np.arange(n, dtype=np.int32)
    seen = False
    for rnd in range(6):
        got = community._leiden_refine(*g, P, v, 1.0, 10, 0, rnd)
        want = ld.refine_round(*g, P, v, 1.0, 10, 0, rnd)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:] and got[2] == n       # (every leaf wants the hub too)
        h = ref.hbit(10, 0, ld.REFINE_ROUND0 + rnd, np.arange(n))
        if h[0] == 1:
            seen = True
            assert got[0][0] == np.flatnonzero(h[1:] == 0)[0] + 1
        else:
            assert got[0][0] == 0
    assert seen


def test_refine_long_rows_share_the_dense_kernel(sa):
    """300 rows longer than the workgroup class: the dense kernel runs at most 128 workgroups, so every one of them takes two or three
    rows in one launch, each on the dense row the one before it used and zeroed again"""
    from sharp_amd import community

    _, block_cap = community._row_caps()
    n, count = block_cap + 60, 300
    g = ref.hubs(n, count)
    assert (np.diff(g[0])[:count] > block_cap).all() and count > 2 * 128
    v = np.arange(n, dtype=np.int32)
    for P in (np.zeros(n, np.int32), (np.arange(n) % 3).astype(np.int32)):
        m0 = check_round(community, g, P, v, rnd=1)[0]
        nxt = ld.refine_round(*g, P, v, 1.0, 10, 0, 1)[0]
        m1 = check_round(community, g, P, nxt, rnd=2)[0]
        assert m0 + m1 > 0


def test_refine_rows_without_an_entry_inside_their_community(sa):
    """vertex 0 of the ring of cliques alone in its community, the rest as the move phase left it: row 0 has entries, none of them
    inside; and the two cliques across a gap, whose community is not connected"""
    from sharp_amd import community

    g = graph("ring")
    P = move_phase("ring").copy()
    P[0] = 179 if (P != 179).all() else 0
    assert (P[g[1][g[0][0]:g[0][1]]] != P[0]).all()
    v = np.arange(len(P), dtype=np.int32)
    for rnd in range(3):
        got = community._leiden_refine(*g, P, v, 1.0, 10, 0, rnd)
        assert got[0][0] == 0
        check_round(community, g, P, v, rnd=rnd)
    rp, col, q, P = ld.cliques_across_a_gap()
    state = np.arange(len(P), dtype=np.int32)
    for rnd in range(12):
        check_round(community, (rp, col, q), P, state, rnd=rnd)
        state = ld.refine_round(rp, col, q, P, state, 1.0, 10, 0, rnd)[0]
    assert np.unique(state).size < len(P) and not np.isin(state[:6], state[6:12]).any()


def test_refine_where_well_connectedness_bites(sa):
    """the noisy planted partition at resolution 8: in its first rounds a sub-community that is not well connected is left out of a
    vertex's candidates, and a vertex alone in its sub-community is not eligible (both found with the reference, asserted here)"""
    from sharp_amd import community

    g = graph("planted")
    gamma = 8.0
    P, states = ref_refinement("planted", gamma)
    excluded = ineligible = 0
    for r in range(4):
        d = {}
        ld.refine_round(*g, P, states[r], gamma, 10, 0, r, detail=d)
        excluded += int(d["excluded"].sum())
        ineligible += int(((np.bincount(states[r], minlength=len(P))[states[r]] == 1) & ~d["eligible"]).sum())
        check_round(community, g, P, states[r], gamma, rnd=r)
    assert excluded > 0 and ineligible > 0
    check_round(community, g, P, states[-1], gamma, rnd=len(states) - 1)


# ---- the components inside a labelling ------------------------------------------------------------------------------------------------
def check_split(community, g, label):
    out, count = community._leiden_split(*g, label)
    want = ld.split(*g[:2], label)
    assert out.dtype == np.int32 and np.array_equal(out, want) and count == np.unique(want).size
    return out


def test_split(sa):
    from sharp_amd import community

    rp, col, q, P = ld.cliques_across_a_gap()
    assert check_split(community, (rp, col, q), P).tolist() == [0] * 6 + [6] * 6 + [12] * 2
    # every community connected: the labelling renamed by its smallest members
    g = graph("blobs")
    P = move_phase("blobs")
    out = check_split(community, g, P)
    low = np.full(len(P), len(P))
    np.minimum.at(low, P, np.arange(len(P)))
    assert np.array_equal(out, low[P])
    check_split(community, g, np.arange(len(P)) % 7)         # scattered labels: many small pieces
    check_split(community, g, np.zeros(len(P), np.int32))    # one label: the graph's components
    check_split(community, graph("path"), np.arange(1025) // 100)
    check_split(community, graph("empty_row"), np.zeros(40, np.int32))
    # self-loops only, and n = 2
    loops = ref.csr_from_pairs(5, np.arange(5), np.arange(5), np.arange(1, 6, dtype=np.int64))
    assert check_split(community, loops, np.zeros(5, np.int32)).tolist() == [0, 1, 2, 3, 4]
    two = graph("two")
    assert check_split(community, two, np.array([1, 1], np.int32)).tolist() == [0, 0]
    assert check_split(community, two, np.array([0, 1], np.int32)).tolist() == [0, 1]
    # the coarse graph of a level, self-loops among its entries
    crp, ccol, cq, new = ref.aggregate(*g, ref_refinement("blobs")[1][-1])
    parent = np.zeros(len(crp) - 1, np.int32)
    parent[new[ref_refinement("blobs")[1][-1]]] = P
    check_split(community, (crp, ccol, cq), parent)


# ---- a level's move phase -------------------------------------------------------------------------------------------------------------
def test_level_from_the_singletons_is_louvains_level(sa):
    from sharp_amd import community

    for name, gamma in (("blobs", 1.0), ("n257", 4.0)):
        g = graph(name)
        n = len(g[0]) - 1
        comm, rounds, Q = community._leiden_level(*g, np.arange(n), gamma)
        want = ref.level(*g, gamma, 10, 0)
        assert np.array_equal(comm, want[0]) and rounds == want[1] and bits(Q) == bits(want[2])


def test_level_from_a_coarse_start(sa):
    from sharp_amd import community

    g = graph("blobs")
    n = len(g[0]) - 1
    for comm0, gamma, level in (((np.arange(n) // 5 * 5), 1.0, 1), (ld.split(*g[:2], np.arange(n) % 3), 0.25, 2), (np.zeros(n, np.int64), 4.0, 0)):
        comm, rounds, Q = community._leiden_level(*g, comm0, gamma, level=level)
        want = ld.level(*g, gamma, 10, level, comm0)
        assert np.array_equal(comm, want[0]) and rounds == want[1] and bits(Q) == bits(want[2])
    comm, rounds, Q = community._leiden_level(*g, np.arange(n) // 5 * 5, max_rounds=3, max_fails=2, tol=1e-3, seed=4)
    want = ld.level(*g, 1.0, 4, 0, np.arange(n) // 5 * 5, tol=1e-3, max_rounds=3, max_fails=2)
    assert np.array_equal(comm, want[0]) and rounds == want[1] == 3 and bits(Q) == bits(want[2])


# ---- the driver -----------------------------------------------------------------------------------------------------------------------
FIELDS = ("n", "communities", "sub_communities", "rounds", "refine_rounds")


def same_run(got, want):
    assert np.array_equal(got["membership"], want["membership"]) and got["membership"].dtype == np.int32
    assert got["n_communities"] == want["n_communities"] and bits(got["modularity"]) == bits(want["modularity"])
    assert len(got["levels"]) == len(want["levels"])
    for g, w in zip(got["levels"], want["levels"]):
        assert tuple(g[f] for f in FIELDS) == tuple(w[f] for f in FIELDS)
        assert bits(g["modularity"]) == bits(w["modularity"])
        if "membership" in g:
            assert np.array_equal(g["membership"], w["membership"] + 1)


@pytest.mark.parametrize("name,gamma", [("blobs", 1.0), ("blobs", 0.25), ("blobs", 4.0), ("gaussian", 1.0), ("path", 1.0), ("planted", 1.0),
                                        ("star", 1.0), ("hubs3", 1.0)])
def test_driver_equals_the_reference(sa, name, gamma):
    """hubs3 holds level-0 rows of the dense class: their dense rows in HBM serve the move and the refine rounds of the level"""
    rp, col, val = float_case(name)
    got = sa.leiden_graph(rp, col, val, resolution=gamma, ret_levels=True)
    same_run(got, ref_run(name, gamma))
    again = sa.leiden_graph(rp, col, val, resolution=gamma)
    assert np.array_equal(got["membership"], again["membership"]) and bits(got["modularity"]) == bits(again["modularity"])
    assert [(bits(l["modularity"]), l["refine_rounds"]) for l in got["levels"]] == [(bits(l["modularity"]), l["refine_rounds"]) for l in again["levels"]]
    assert bits(sa.modularity(rp, col, val, got["membership"], gamma)) == bits(got["modularity"])


def test_driver_limits(sa):
    rp, col, val = float_case("blobs")
    one = sa.leiden_graph(rp, col, val, max_levels=1, ret_levels=True)
    same_run(one, ld.leiden(rp, col, val, max_levels=1))
    assert len(one["levels"]) == 1 and one["levels"][0]["sub_communities"] < 1500
    cut = sa.leiden_graph(rp, col, val, max_refine_rounds=1, seed=4)
    same_run(cut, ld.leiden(rp, col, val, 1.0, 4, max_refine_rounds=1))
    assert all(l["refine_rounds"] <= 1 for l in cut["levels"]) and cut["levels"][0]["refine_rounds"] == 1
    assert ref_run("blobs", 1.0)["levels"][0]["refine_rounds"] > 1
    other = sa.leiden_graph(rp, col, val, max_rounds=3, max_fails=2, tol=1e-3)
    same_run(other, ld.leiden(rp, col, val, max_rounds=3, max_fails=2, tol=1e-3))


def test_the_result_is_connected_when_the_level_cap_ends_the_run(sa):
    """max_levels = 2 on the unstructured graph: the run ends while the refinement still merges, and the second level's P is split"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components

    rp, col, val = float_case("gaussian")
    got = sa.leiden_graph(rp, col, val, resolution=4.0, max_levels=2)
    same_run(got, ld.leiden(rp, col, val, 4.0, max_levels=2))
    m = got["membership"]
    row = np.repeat(np.arange(len(m)), np.diff(rp))
    keep = m[row] == m[col]
    comp = connected_components(csr_matrix((np.ones(int(keep.sum())), (row[keep], col[keep])), shape=(len(m), len(m))), directed=False)[1]
    assert np.unique(np.stack([m, comp]), axis=1).shape[1] == got["n_communities"]


# ---- front doors ----------------------------------------------------------------------------------------------------------------------
def test_front_doors_agree(sa):
    import importlib

    um = importlib.import_module("sharp_amd.umap")               # (sharp_amd.umap is the function)
    X = ref.blobs_graph()[4]
    a = sa.leiden(X, ret_nn=True, ret_levels=True)
    nb = sa.knn(X, 14)
    assert np.array_equal(a["nn"]["index"], nb[0]) and np.array_equal(a["nn"]["distance"], nb[1])
    b = sa.leiden_neighbors(*nb, ret_levels=True)
    c = sa.leiden_graph(*um._graph(*nb)[:3], ret_levels=True)
    d = sa.leiden_neighbors(nb[0], nb[1] ** 2, squared=True)
    for other in (b, c):
        same_run(a, dict(other, levels=[dict(l, membership=l["membership"] - 1) for l in other["levels"]]))
    assert np.array_equal(a["membership"], d["membership"])
    assert ref.adjusted_rand(a["membership"], ref.blobs_graph()[3]) == 1.0
    assert bits(sa.modularity(*um._graph(*nb)[:3], a["membership"])) == bits(a["modularity"])
    assert a["seed"] == 10 and a["n_communities"] == int(a["membership"].max())
    # the SNN graph
    s = sa.leiden(X, graph="snn", ret_levels=True)
    t = sa.leiden_snn(nb[0], ret_levels=True)
    g = sa.snn_graph(nb[0])
    u = sa.leiden_graph(g["row_ptr"], g["col"], g["val"], ret_levels=True)
    for other in (t, u):
        same_run(s, dict(other, levels=[dict(l, membership=l["membership"] - 1) for l in other["levels"]]))
    w = sa.leiden(X, graph="snn", prune=0.2, resolution=2.0, max_refine_rounds=3)
    same_run(w, sa.leiden_snn(nb[0], 0.2, resolution=2.0, max_refine_rounds=3))


# ---- Louvain is unchanged -------------------------------------------------------------------------------------------------------------
def test_louvain_after_a_leiden_call(sa):
    rp, col, val = float_case("blobs")
    sa.leiden_graph(rp, col, val, resolution=4.0)
    got = sa.louvain_graph(rp, col, val, resolution=4.0, ret_levels=True)
    want = ref.louvain(rp, col, val, 4.0)
    assert np.array_equal(got["membership"], want["membership"]) and bits(got["modularity"]) == bits(want["modularity"])
    assert [(l["n"], l["communities"], l["rounds"], bits(l["modularity"])) for l in got["levels"]] == \
        [(l["n"], l["communities"], l["rounds"], bits(l["modularity"])) for l in want["levels"]]
    for g, w in zip(got["levels"], want["levels"]):
        assert np.array_equal(g["membership"], w["membership"] + 1)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_message(sa):
    rp, col, val = float_case("ring")
    bad = val.copy()
    bad[0] = 2.0
    with pytest.raises(sa.SharpError, match="leiden_graph: the graph is not symmetric"):
        sa.leiden_graph(rp, col, bad)
    with pytest.raises(sa.SharpError, match="no positive weight"):
        sa.leiden_graph(rp, col, np.zeros_like(val))
    with pytest.raises(sa.SharpError, match="max_refine_rounds must be in 1 .. 100000"):
        sa.leiden_graph(rp, col, val, max_refine_rounds=0)
    nb = sa.knn(ref.blobs_graph()[4], 5)
    idx = nb[0].copy()
    idx[7, 2] = 7
    with pytest.raises(sa.SharpError, match="leiden_neighbors: .*itself"):
        sa.leiden_neighbors(idx, nb[1])
    import _snn_ref

    with pytest.raises(sa.SharpError, match="leiden_snn: .*holds no positive weight"):
        sa.leiden_snn(_snn_ref.ring(64, 1), 1.0)               # K = 1 ring: no two rows have equal sets
    # the library refuses what reaches it without the package's checks
    import ctypes as C

    from sharp_amd import community
    from sharp_amd._lib import f64, i32, i64, lib
    n = len(rp) - 1

    def call(values, resolution=1.0, max_refine_rounds=200, max_rounds=200):
        o = community._Out(n, 20, False, True)
        return lib().sharp_leiden_graph(i64(rp), i32(col), f64(values), n, resolution, 1e-7, 20, max_rounds, 4, max_refine_rounds, 10.0, *o.args())

    assert call(val) == 0
    for kw, text in ((dict(values=bad), b"leiden_graph: the graph is not symmetric"), (dict(values=val, resolution=0.0), b"resolution must be in"),
                     (dict(values=val, max_rounds=0), b"max_rounds must be in"), (dict(values=val, max_refine_rounds=0), b"max_refine_rounds must be in"),
                     (dict(values=val, max_refine_rounds=100001), b"max_refine_rounds must be in")):
        assert call(**kw) != 0 and text in lib().sharp_last_error()
    g = graph("ring")
    prop, m, w = np.zeros(n, np.int32), C.c_longlong(), C.c_longlong()
    P = np.zeros(n, np.int32)
    out_of_range = P.copy()
    out_of_range[3] = n
    for Pa, ra in ((out_of_range, P), (P, out_of_range)):
        rc = lib().sharp_leiden_refine(i64(g[0]), i32(g[1]), i64(g[2]), n, i32(Pa), i32(ra), 1.0, 10.0, 0, 0, i32(prop), C.byref(m), C.byref(w))
        assert rc != 0 and b"a community id outside [0, n)" in lib().sharp_last_error()
    rc = lib().sharp_leiden_refine(i64(g[0]), i32(g[1]), i64(g[2]), n, i32(P), i32(P), 1.0, 10.0, 0, 100000, i32(prop), C.byref(m), C.byref(w))
    assert rc != 0 and b"round in 0 .. 99999" in lib().sharp_last_error()
