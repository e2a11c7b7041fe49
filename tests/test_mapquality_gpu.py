"""Neighbour ranks, trustworthiness and continuity on the MI355X against the numpy specification (tests/_mapquality_ref.py, DESIGN.md
§17).  Everything the device computes is an integer: every comparison of ranks and penalties is exact, the scores are the reference's
floats bit for bit, and sklearn is met within rounding.  The shapes are the smallest at which each part can go wrong: n no multiple of
the 64-row tile, several column parts, every slice width (K = 15: 16, K = 30: 32, K = 90 and 255: two and four slices of 64), one to
three feature panels with the last one partial, and a launch split at a row count that is no multiple of the tile."""
import ctypes as C

import numpy as np
import pytest

import _mapquality_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


# ---- ties, duplicates, self -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 15, 30, 90, 255])
def test_lattice_ranks_equal_the_reference(sa, K):
    """integers 0 .. 3 in 3 columns, 257 rows: exact ties in every row (the lower index first), rows at distance 0 off the diagonal, the
    skipped diagonal, n = 4 * 64 + 1, every slice width and K above one slice"""
    X = ref.lattice()
    idx = ref.random_lists(257, K, 40 + K)
    got = sa.neighbor_ranks(X, idx)
    assert got.dtype == np.int32 and got.shape == (257, K)
    want = ref.ranks(X, idx)
    assert got.min() >= 1 and got.max() <= 256
    assert np.array_equal(got, want)
    s = np.sort(got, axis=1)                                       # different rows never share a rank, tied or not
    assert (s[:, 1:] > s[:, :-1]).all()


# ---- widths ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [15, 90])
@pytest.mark.parametrize("d", [3, 10, 50, 70])
def test_gaussian_ranks_equal_the_reference(sa, d, K):
    """1 025 x d: one panel of features (partial), one and a half, and three with the last one partial"""
    X = ref.gaussian(1025, d, 200 + d)
    idx = ref.random_lists(1025, K, 300 + d + K)
    assert np.array_equal(sa.neighbor_ranks(X, idx), ref.ranks(X, idx))


# ---- against the exact search ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    return ref.blobs(20011, 10, 3)                                 # (tests/_knn_descent_ref.py: full_input("blobs20011"))


def test_ranks_of_the_exact_lists_are_one_to_k(sa, big):
    """needs no CPU reference: knn()'s K nearest rows, in knn()'s order, have the ranks 1 .. K -- the kernel's distances and tie rule are
    knn()'s.  A split into launches of 5 004 rows (no multiple of the tile) changes nothing."""
    K = 15
    idx, _ = sa.knn(big, K)
    got = sa.neighbor_ranks(big, idx)
    assert np.array_equal(got, np.broadcast_to(np.arange(1, K + 1, dtype=np.int32), got.shape))
    assert np.array_equal(sa.neighbor_ranks(big, idx, max_rows_per_launch=5004), got)


def test_random_lists_on_sampled_rows(sa, big):
    K = 15
    idx = ref.random_lists_large(20011, K, 5)
    got = sa.neighbor_ranks(big, idx)
    rows = np.sort(np.random.default_rng(6).choice(20011, size=512, replace=False))
    assert np.array_equal(got[rows], ref.ranks(big, idx, rows=rows))
    assert np.array_equal(sa.neighbor_ranks(big, idx, max_rows_per_launch=5004), got)
    assert np.array_equal(sa.neighbor_ranks(big, idx), got)        # two calls, the same bits


# ---- scores ---------------------------------------------------------------------------------------------------------------------------
def test_scores_equal_the_reference_and_meet_sklearn(sa):
    manifold = pytest.importorskip("sklearn.manifold")
    K = 15
    X = ref.blobs(1025, 10, 1)
    Y = ref.map_of(X, 11)
    for name, fn, rfn, a, b, listed in (("trustworthiness", sa.trustworthiness, ref.trustworthiness, X, Y, Y),
                                        ("continuity", sa.continuity, ref.continuity, Y, X, X)):
        want, pen = rfn(X, Y, K)
        got = fn(X, Y, n_neighbors=K, ret_points=True)
        assert got["n_neighbors"] == K and got["penalty"].dtype == np.int64 and got["points"].dtype == np.float64
        assert np.array_equal(got["penalty"], pen)
        assert got["score"] == want and fn(X, Y, n_neighbors=K) == want
        assert np.array_equal(got["points"], ref.points(pen, 1025, K))
        sk = manifold.trustworthiness(a, b, n_neighbors=K)
        print(f"{name}: GPU {got['score']!r}, reference {want!r}, sklearn {sk!r}")
        assert abs(got["score"] - sk) <= 1e-12
        # the lists supplied: the bits of not supplying them
        lists = sa.knn(listed, K)
        assert fn(X, Y, neighbors=lists) == want and fn(X, Y, neighbors=lists[0], n_neighbors=3) == want
        assert np.array_equal(fn(X, Y, neighbors=lists, ret_points=True)["penalty"], pen)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_umap_map_end_to_end(sa):
    """a short umap run on the 1 500 x 10 blobs of DESIGN.md §13: the score on the GPU's own lists is the reference's, sklearn (which
    selects the map's neighbours from GEMM-form distances) is met within 1e-9, and continuity from the lists umap hands back is
    continuity computed from X"""
    import _umap_ref

    manifold = pytest.importorskip("sklearn.manifold")
    X, _ = _umap_ref.blobs()
    X = np.ascontiguousarray(X)
    res = sa.umap(X, n_neighbors=15, n_epochs=30, ret_nn=True)
    Y = np.ascontiguousarray(res["Y"], np.float64)
    assert Y.shape == (1500, 2)
    K = 15
    t = sa.trustworthiness(X, Y, n_neighbors=K)
    want, _ = ref.trustworthiness(X, Y, K, lists=sa.knn(Y, K)[0])
    sk = manifold.trustworthiness(X, Y, n_neighbors=K)
    print(f"umap map after 30 epochs: trustworthiness GPU {t!r}, sklearn {sk!r}")
    assert t == want
    assert abs(t - sk) <= 1e-9
    nn = res["nn"]
    Kn = np.asarray(nn["index"]).shape[1]
    assert Kn == 14
    c = sa.continuity(X, Y, neighbors=nn)
    assert c == sa.continuity(X, Y, n_neighbors=Kn)
    assert c == sa.continuity(X, Y, neighbors=(nn["index"], nn["distance"]))
    assert abs(c - manifold.trustworthiness(Y, X, n_neighbors=Kn)) <= 1e-9


# ---- other ----------------------------------------------------------------------------------------------------------------------------
def test_dotc_twin(sa):
    """the .C() convention: every argument a pointer, n as a double, the status last; equal to the plain entry's output"""
    L = sa.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)                                     # noqa: E731
    I = lambda *v: np.array(v, np.int32)                                           # noqa: E731
    n, d, K = 257, 10, 15
    X = ref.gaussian(n, d, 8)
    idx = ref.random_lists(n, K, 9)
    want = sa.neighbor_ranks(X, idx)
    out, st = np.zeros((n, K), np.int32), I(-1)
    L.sharp_C_neighbor_ranks(P(X), P(np.array([float(n)])), P(I(d)), P(I(K)), P(idx), P(I(0)), P(out), P(st))
    assert st[0] == 0 and np.array_equal(out, want)
    st[0] = -1
    L.sharp_C_neighbor_ranks(P(X), P(np.array([float(n)])), P(I(d)), P(I(K)), P(idx), P(I(100)), P(out), P(st))
    assert st[0] == 0 and np.array_equal(out, want)
    bad = idx.copy()
    bad[200, 3] = 200
    L.sharp_C_neighbor_ranks(P(X), P(np.array([float(n)])), P(I(d)), P(I(K)), P(bad), P(I(0)), P(out), P(st))
    assert st[0] != 0 and b"names itself" in L.sharp_last_error() and b"row 200" in L.sharp_last_error()


def test_refusals(sa):
    n, K = 300, 15
    X = ref.gaussian(n, 6, 1)
    Y = ref.map_of(X, 2)
    idx = ref.random_lists(n, K, 3)
    E = sa.SharpError
    with pytest.raises(E, match=r"n_neighbors \(150\) should be less than n_samples / 2 \(150.0\)"):
        sa.trustworthiness(X, Y, n_neighbors=150)
    with pytest.raises(E, match=r"n_neighbors \(150\) should be less than n_samples / 2"):
        sa.continuity(X, Y, n_neighbors=150)
    with pytest.raises(E, match="at most 255 neighbours"):
        sa.neighbor_ranks(ref.gaussian(600, 2, 1), ref.random_lists(600, 256, 1))
    out = np.zeros((600, 256), np.int32)                           # (the library's own refusal, past the Python check)
    x600 = ref.gaussian(600, 2, 1)
    assert sa.lib().sharp_neighbor_ranks(x600.ctypes.data, 600, 2, 2, 256, ref.random_lists(600, 256, 1).ctypes.data, 0, out.ctypes.data) != 0
    assert b"K must be in 1 .. 255" in sa.lib().sharp_last_error()
    for value in (n, -1, 2 ** 31 + 5):
        bad = idx.astype(np.int64)
        bad[123, 4] = value
        with pytest.raises(E, match=r"a neighbour index outside \[0, n\) \(row 123, counted from 0\)"):
            sa.neighbor_ranks(X, bad)
    bad = idx.copy()
    bad[77, 0] = 77
    with pytest.raises(E, match=r"a row names itself as a neighbour \(row 77, counted from 0\)"):
        sa.neighbor_ranks(X, bad)
    with pytest.raises(E, match=r"a row names itself as a neighbour \(row 77"):
        sa.trustworthiness(X, Y, neighbors=bad)
    bad = idx.copy()
    bad[299, 14] = bad[299, 2]
    bad[150, 1] = bad[150, 0]
    with pytest.raises(E, match=r"the same neighbour index twice in a row \(row 150, counted from 0\)"):
        sa.neighbor_ranks(X, bad)
    for v in (np.nan, np.inf, -1e101):
        bx = X.copy()
        bx[299, 5] = v
        with pytest.raises(E, match=r"NA / NaN / Inf or a value beyond 1e100 \(row 300, column 6\)"):
            sa.neighbor_ranks(bx, idx)
        with pytest.raises(E, match=r"row 300, column 6"):
            sa.continuity(Y, bx, n_neighbors=5)
    out = np.zeros((n, K), np.int32)                               # (the library's own check, past the Python one)
    bx = X.copy()
    bx[5, 0] = np.nan
    assert sa.lib().sharp_neighbor_ranks(bx.ctypes.data, n, 6, 6, K, idx.ctypes.data, 0, out.ctypes.data) != 0
    assert b"(row 6, column 1)" in sa.lib().sharp_last_error()
    with pytest.raises(E, match="X has 300 rows and Y 299"):
        sa.trustworthiness(X, Y[:299])
    with pytest.raises(E, match="X has 300 rows and Y 299"):
        sa.continuity(X, Y[:299])
    with pytest.raises(E, match="need n >= 3 rows"):
        sa.neighbor_ranks(X[:2], np.array([[1], [0]], np.int32))
    two = np.array([[1], [0]], np.int32)
    assert sa.lib().sharp_neighbor_ranks(X.ctypes.data, 2, 6, 6, 1, two.ctypes.data, 0, out.ctypes.data) != 0
    assert b"need n >= 3 rows" in sa.lib().sharp_last_error()
    # and the smallest input there is
    tiny = np.array([[0.0], [1.0], [3.0]])
    assert np.array_equal(sa.neighbor_ranks(tiny, np.array([[2, 1], [0, 2], [0, 1]], np.int32)), [[2, 1], [1, 2], [2, 1]])
