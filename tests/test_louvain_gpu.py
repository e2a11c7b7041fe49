"""Louvain on the MI355X against the numpy specification (tests/_louvain_ref.py), stage by stage and end to end.  Every
comparison is exact: weights are integers, the gains and the modularity are fp64 expressions in a stated operation order, and the sum
of the modularity's terms runs in a fixed order.  The shapes are the smallest at which each part can go wrong: rows of exactly the
longest length of each row class of the move kernel and one more, a table as full as it gets (every neighbour its own community) and
one with few keys that many lanes add to, an empty row, n = 2, a sort key that needs more than 32 bits."""
import functools

import numpy as np
import pytest

import _louvain_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


def bits(x):
    return np.float64(x).tobytes()


@functools.lru_cache(maxsize=None)
def float_case(name):
    """(rp, col, val) of the float-weighted cases; computed once and left alone"""
    if name == "blobs":
        return ref.blobs_graph()[:3]
    if name == "gaussian":
        return ref.gaussian_graph()[:3]
    if name == "path":
        return ref.path()
    if name == "planted":
        return ref.planted()[:3]
    if name == "star":
        return ref.star()
    if name == "ring":
        return ref.ring_of_cliques()
    if name == "star3100":                                   # a level-0 row beyond the workgroup class: the dense kernel in the driver
        return ref.star(3100)
    if name == "hubs3":                                      # three such rows and a ring, random weights
        return ref.hubs(3140, 3, seed=6, dtype=np.float64)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def int_case(name):
    """(rp, col, q) of a level's graph"""
    if name in ("blobs", "path", "star", "ring"):
        rp, col, val = float_case(name)
        return ref.drop_zeros(rp, col, ref.quantise(rp, col, val)[0])
    if name == "complete":
        return ref.complete_int()
    if name == "empty_row":                                  # a path and a vertex without entries in the middle of the ids
        rp, col, q = ref.csr_from_pairs(40, np.r_[np.arange(0, 19), np.arange(21, 39)], np.r_[np.arange(1, 20), np.arange(22, 40)],
                                        np.arange(1, 38, dtype=np.int64))
        return rp, col, q
    if name == "two":
        return ref.csr_from_pairs(2, [0], [1], np.array([5], np.int64))
    if name == "n257":
        rng = np.random.default_rng(11)
        i, j = np.triu_indices(257, 1)
        keep = rng.random(i.size) < 0.05
        return ref.csr_from_pairs(257, i[keep], j[keep], rng.integers(1, 100, size=int(keep.sum())).astype(np.int64))
    if name.startswith("hub"):
        return ref.hub(int(name[3:]))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ref_run(name, gamma):
    return ref.louvain(*float_case(name), gamma)


def states(n):
    """memberships a round may start from: the singletons (every neighbour a key of its own), a few large communities (many lanes add to
    one key), and scattered ids"""
    v = np.arange(n)
    return {"singletons": v.astype(np.int32), "mod7": (v % 7).astype(np.int32), "blocks": (v // 5 * 5).astype(np.int32)}


# ---- quantise -------------------------------------------------------------------------------------------------------------------------
def test_quantise_equals_the_reference(sa):
    from sharp_amd import community

    rp, col, val = float_case("blobs")
    q, k, m2 = community._quantise(rp, col, val)
    rq, rk, rm2 = ref.quantise(rp, col, val)
    assert q.dtype == np.int64 and np.array_equal(q, rq) and np.array_equal(k, rk) and m2 == rm2
    assert q.max() == 1 << 24 and q.min() >= 0


def test_quantise_drops_the_smallest_weights(sa):
    """weights down to 2^-30 of the largest: below 2^-25 they round to 0 and leave the graph; a tie at one half rounds to even"""
    from sharp_amd import community

    n = 64
    a = np.arange(n - 1)
    w = 2.0 ** -(a % 32).astype(np.float64)
    w[5] = 1.5 * 2.0 ** -24                                  # q = 1.5 -> 2
    w[6] = 2.5 * 2.0 ** -24                                  # q = 2.5 -> 2
    w[7] = 0.5 * 2.0 ** -24                                  # q = 0.5 -> 0
    rp, col, val = ref.csr_from_pairs(n, a, a + 1, w)
    q, k, m2 = community._quantise(rp, col, val)
    rq, rk, rm2 = ref.quantise(rp, col, val)
    assert (rq == 0).sum() >= 12 and np.array_equal(q, rq) and np.array_equal(k, rk) and m2 == rm2
    # the driver drops them: the same run as on the graph without them
    got = sa.louvain_graph(rp, col, val, ret_levels=True)
    want = ref.louvain(rp, col, val)
    assert np.array_equal(got["membership"], want["membership"]) and bits(got["modularity"]) == bits(want["modularity"])


# ---- move -----------------------------------------------------------------------------------------------------------------------------
def check_move(community, rp, col, q, comm, gamma=1.0, level=0, rnd=0, seed=10):
    got = community._move(rp, col, q, comm, gamma, seed, level, rnd)
    want = ref.move(rp, col, q, comm, gamma, seed, level, rnd)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    return int((got != comm).sum())


@pytest.mark.parametrize("name", ["blobs", "path", "ring", "star", "complete", "empty_row", "two", "n257"])
def test_move_from_singletons(sa, name):
    from sharp_amd import community

    rp, col, q = int_case(name)
    n = len(rp) - 1
    rounds = 12 if n < 100 else 3                            # (a pair is open in a quarter of the rounds: few vertices need more of them)
    moved = sum(check_move(community, rp, col, q, np.arange(n, dtype=np.int32), rnd=r) for r in range(rounds))
    assert moved > 0


@pytest.mark.parametrize("name", ["blobs", "complete", "n257", "star"])
@pytest.mark.parametrize("state", ["mod7", "blocks"])
def test_move_from_coarser_states(sa, name, state):
    from sharp_amd import community

    rp, col, q = int_case(name)
    comm = states(len(rp) - 1)[state]
    for gamma, level, rnd in ((1.0, 0, 0), (0.25, 1, 3), (4.0, 2, 7)):
        check_move(community, rp, col, q, comm, gamma, level, rnd)


def test_move_after_five_reference_rounds(sa):
    from sharp_amd import community

    rp, col, q = int_case("blobs")
    comm, rounds, _ = ref.level(rp, col, q, 1.0, 10, 0, max_rounds=5)
    assert rounds == 5 and np.unique(comm).size < len(rp) - 1
    check_move(community, rp, col, q, comm, rnd=5)
    check_move(community, rp, col, q, comm, rnd=6)


def test_move_at_every_row_class_boundary(sa):
    """a row of exactly the longest length of the wave class and of the workgroup class, and one entry more: from the singletons (as
    many keys as entries) and from a few communities"""
    from sharp_amd import community

    wave_cap, block_cap = community._row_caps()
    assert 64 <= wave_cap < block_cap
    for length in (wave_cap, wave_cap + 1, block_cap, block_cap + 1):
        rp, col, q = int_case(f"hub{length}")
        assert rp[1] - rp[0] == length
        for comm in states(len(rp) - 1).values():
            for rnd in (0, 1):
                check_move(community, rp, col, q, comm, rnd=rnd)


def test_move_long_rows_share_the_dense_kernel(sa):
    """300 rows longer than the workgroup class: the dense kernel runs at most 128 workgroups, so every one of them takes two or three
    rows in one launch, each on the dense row the one before it used and zeroed again"""
    from sharp_amd import community

    _, block_cap = community._row_caps()
    n, count = block_cap + 60, 300
    rp, col, q = ref.hubs(n, count)
    assert (np.diff(rp)[:count] > block_cap).all() and count > 2 * 128
    for comm in states(n).values():
        check_move(community, rp, col, q, comm, rnd=1)
        check_move(community, rp, col, q, comm, rnd=2)


# ---- modularity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blobs", "path", "complete", "empty_row", "two", "n257"])
def test_modularity_equals_the_reference(sa, name):
    from sharp_amd import community

    rp, col, q = int_case(name)
    n = len(rp) - 1
    cases = dict(states(n), one=np.zeros(n, np.int32))
    for gamma in (1.0, 0.25):
        for comm in cases.values():
            assert bits(community._modularity_q(rp, col, q, comm, gamma)) == bits(ref.modularity_q(rp, col, q, comm, gamma))
    assert community._modularity_q(rp, col, q, cases["one"], 1.0) == 0.0       # in = tot = 2m: 1 - 1


def test_public_modularity(sa):
    rp, col, val = float_case("blobs")
    lab = np.arange(1500) % 6 + 1
    assert bits(sa.modularity(rp, col, val, lab)) == bits(ref.modularity(rp, col, val, lab))
    assert bits(sa.modularity(rp, col, val, lab * 10 - 3, 0.5)) == bits(ref.modularity(rp, col, val, lab, 0.5))


# ---- aggregate ------------------------------------------------------------------------------------------------------------------------
def check_aggregate(community, rp, col, q, comm):
    got = community._aggregate(rp, col, q, comm)
    want = ref.aggregate(rp, col, q, comm)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert int(got[2].sum()) == int(np.asarray(q).sum())
    return got


def test_aggregate_identity_needs_a_wide_key(sa):
    from sharp_amd import community

    rp, col, q = ref.path(70001, np.int64)
    assert 70001 ** 2 > 1 << 32
    out = check_aggregate(community, rp, col, q, np.arange(70001, dtype=np.int32))
    assert np.array_equal(out[0], rp) and np.array_equal(out[1], col)


def test_aggregate_into_one_and_twice(sa):
    from sharp_amd import community

    rp, col, q = int_case("blobs")
    n = len(rp) - 1
    one = check_aggregate(community, rp, col, q, np.full(n, 3, np.int32))
    assert one[0].tolist() == [0, 1] and one[1].tolist() == [0] and one[2].tolist() == [int(q.sum())]
    a = check_aggregate(community, rp, col, q, (np.arange(n) // 5 * 5).astype(np.int32))
    m = len(a[0]) - 1
    b = check_aggregate(community, a[0], a[1], a[2], (np.arange(m) % 9).astype(np.int32))      # self-loops accumulate
    assert len(b[0]) - 1 == 9 and (b[2][b[1] == np.repeat(np.arange(9), np.diff(b[0]))] > 0).all()
    check_aggregate(community, *int_case("empty_row"), np.arange(40, dtype=np.int32))


# ---- the driver -----------------------------------------------------------------------------------------------------------------------
def same_run(got, want):
    assert np.array_equal(got["membership"], want["membership"]) and got["membership"].dtype == np.int32
    assert got["n_communities"] == want["n_communities"] and bits(got["modularity"]) == bits(want["modularity"])
    assert len(got["levels"]) == len(want["levels"])
    for g, w in zip(got["levels"], want["levels"]):
        assert (g["n"], g["communities"], g["rounds"]) == (w["n"], w["communities"], w["rounds"])
        assert bits(g["modularity"]) == bits(w["modularity"])
        if "membership" in g:
            assert np.array_equal(g["membership"], w["membership"] + 1)


@pytest.mark.parametrize("name,gamma", [("blobs", 1.0), ("blobs", 0.25), ("blobs", 4.0), ("gaussian", 1.0), ("path", 1.0), ("planted", 1.0),
                                        ("star", 1.0), ("star3100", 1.0), ("hubs3", 1.0), ("hubs3", 3.0)])
def test_driver_equals_the_reference(sa, name, gamma):
    """star3100 and hubs3 hold level-0 rows of the dense class: their dense rows in HBM serve every round of the level"""
    rp, col, val = float_case(name)
    got = sa.louvain_graph(rp, col, val, resolution=gamma, ret_levels=True)
    same_run(got, ref_run(name, gamma))
    again = sa.louvain_graph(rp, col, val, resolution=gamma)
    assert np.array_equal(got["membership"], again["membership"]) and bits(got["modularity"]) == bits(again["modularity"])
    assert [bits(l["modularity"]) for l in got["levels"]] == [bits(l["modularity"]) for l in again["levels"]]
    assert bits(sa.modularity(rp, col, val, got["membership"], gamma)) == bits(got["modularity"])


def test_driver_limits(sa):
    rp, col, val = float_case("blobs")
    one = sa.louvain_graph(rp, col, val, max_levels=1)
    same_run(one, ref.louvain(rp, col, val, max_levels=1))
    assert len(one["levels"]) == 1 and one["n_communities"] == ref_run("blobs", 1.0)["levels"][0]["communities"]
    cut = sa.louvain_graph(rp, col, val, max_rounds=3, seed=4)
    same_run(cut, ref.louvain(rp, col, val, 1.0, 4, max_rounds=3))
    assert cut["levels"][0]["rounds"] == 3
    assert ref_run("blobs", 1.0)["levels"][0]["rounds"] > 3
    other = sa.louvain_graph(rp, col, val, max_fails=2, tol=1e-3)
    same_run(other, ref.louvain(rp, col, val, max_fails=2, tol=1e-3))


# ---- front doors ----------------------------------------------------------------------------------------------------------------------
def test_front_doors_agree(sa):
    import importlib

    um = importlib.import_module("sharp_amd.umap")               # (sharp_amd.umap is the function)
    X = ref.blobs_graph()[4]
    a = sa.louvain(X, ret_nn=True, ret_levels=True)
    nb = sa.knn(X, 14)
    assert np.array_equal(a["nn"]["index"], nb[0]) and np.array_equal(a["nn"]["distance"], nb[1])
    b = sa.louvain_neighbors(*nb, ret_levels=True)
    c = sa.louvain_graph(*um._graph(*nb)[:3], ret_levels=True)
    d = sa.louvain_neighbors(nb[0], nb[1] ** 2, squared=True)
    for other in (b, c):
        same_run(a, dict(other, levels=[dict(l, membership=l["membership"] - 1) for l in other["levels"]]))
    assert np.array_equal(a["membership"], d["membership"])
    assert ref.adjusted_rand(a["membership"], ref.blobs_graph()[3]) == 1.0
    g = um._graph(*nb)[:3]
    assert bits(sa.modularity(*g, a["membership"])) == bits(a["modularity"])
    assert a["seed"] == 10 and a["n_communities"] == int(a["membership"].max())
    sizes = np.bincount(a["membership"])[1:]
    assert (np.diff(sizes) <= 0).all()                        # 1 .. G by decreasing size


def test_descent_front_door(sa):
    X = ref.blobs_graph()[4]
    a = sa.louvain(X, nn_method="descent", ret_nn=True)
    idx, dist = sa.knn_descent(X, 14)
    assert a["nn"]["method"] == "descent" and np.array_equal(a["nn"]["index"], idx)
    b = sa.louvain_neighbors(idx, dist)
    assert np.array_equal(a["membership"], b["membership"]) and bits(a["modularity"]) == bits(b["modularity"])


def test_refusals_by_message(sa):
    rp, col, val = float_case("ring")
    bad = val.copy()
    bad[0] = 2.0
    with pytest.raises(sa.SharpError, match="not symmetric"):
        sa.louvain_graph(rp, col, bad)
    bad = val.copy()
    bad[3] = np.nan
    with pytest.raises(sa.SharpError, match="NA / NaN / Inf"):
        sa.louvain_graph(rp, col, bad)
    with pytest.raises(sa.SharpError, match="no positive weight"):
        sa.louvain_graph(rp, col, np.zeros_like(val))
    with pytest.raises(sa.SharpError, match="resolution must be in"):
        sa.louvain_graph(rp, col, val, resolution=0.0)
    nb = sa.knn(ref.blobs_graph()[4], 5)
    idx = nb[0].copy()
    idx[7, 2] = 7
    with pytest.raises(sa.SharpError, match="louvain_neighbors: .*itself"):
        sa.louvain_neighbors(idx, nb[1])
    # the library refuses what reaches it without the package's checks
    import ctypes as C

    from sharp_amd._lib import f64, i32, i64, lib
    n = len(rp) - 1
    mem, ln, lc, lr, lq, nl = np.zeros(n, np.int32), np.zeros(20, np.int64), np.zeros(20, np.int64), np.zeros(20, np.int32), np.zeros(20), C.c_int()
    bad = val.copy()
    bad[0] = 2.0
    rc = lib().sharp_louvain_graph(i64(rp), i32(col), f64(bad), n, 1.0, 1e-7, 20, 200, 4, 10.0, i32(mem), 20, i64(ln), i64(lc), i32(lr), f64(lq),
                                   C.byref(nl), None)
    assert rc != 0 and b"not symmetric" in lib().sharp_last_error()
