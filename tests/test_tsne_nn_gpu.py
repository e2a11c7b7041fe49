"""t-SNE from given distances (Rtsne(is_distance=True), sharp_tsne_dist) and from given neighbours (Rtsne_neighbors,
sharp_tsne_neighbors) on the MI355X, against tests/_tsne_nn_ref.py and against the direct path."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial.distance import cdist

import _snn_ref
import _tsne_nn_ref as nn
import _tsne_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


def _blobs(n, d, groups, seed, spread=0.3):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 3, size=(groups, d))
    return centres[rng.integers(0, groups, n)] + spread * rng.normal(size=(n, d))


def _int_data(n, p, seed):
    x = np.random.default_rng(seed).integers(0, 4, size=(n, p)).astype(np.float64)
    x[n // 2] = x[3]                                                 # three copies: zero distances, equal rows of D
    x[n - 1] = x[3]
    x[n // 3] = x[11]
    return x


# ---- 1. selection from distances ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,Ks", [(1025, (64, 90, 255)), (256, (255,))])
def test_selection_from_distances_is_exact(sa, n, Ks):
    """manhattan distances of small integers: every distance an exact integer, ties plentiful.  n = 1025 is one past a 64-column stride
    and past the 128 padding of the matrix; K = 255 fills four strides of the list, the last short by one; n = 256, K = 255 makes every
    other object a neighbour."""
    x = _int_data(n, 37, 41)
    d = sa.dist(x, "manhattan")
    D = nn.square_form(d, n)
    assert np.array_equal(D, cdist(x, x, "cityblock"))
    for K in Ks:
        ridx, rdist = nn.knn_from_dist(D, K)
        idx, dist = sa.knn(d, K, is_distance=True)
        assert idx.dtype == np.int32 and idx.shape == (n, K)
        assert np.array_equal(idx, ridx)
        assert np.array_equal(dist, rdist)                           # bit for bit D[i, idx]
        i2, d2 = sa.knn(d, K, is_distance=True, squared=True)
        assert np.array_equal(i2, ridx) and np.array_equal(d2, rdist * rdist)
    im, dm = sa.knn(D, Ks[-1], is_distance=True)                     # the square-matrix form
    assert np.array_equal(im, idx) and np.array_equal(dm, dist)


def test_knn_from_rows_is_the_library_knn(sa):
    X = _blobs(700, 9, 4, 42)
    ridx, rd2 = ref.knn(X, 30)
    idx, d2 = sa.knn(X, 30, squared=True)
    assert np.array_equal(idx, ridx)
    np.testing.assert_allclose(d2, rd2, rtol=1e-12, atol=1e-300)
    i1, d1 = sa.knn(X, 30)
    assert np.array_equal(i1, idx) and np.array_equal(d1, np.sqrt(d2))


# ---- 2. P from neighbours ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blobs1500():
    return _blobs(1500, 30, 5, 13)


@pytest.mark.parametrize("perplexity,K", [(30, 90), (85, 255), (20, 64)])
def test_affinities_from_neighbours_match_reference(sa, blobs1500, perplexity, K):
    from sharp_amd import tsne

    idx, d2 = sa.knn(blobs1500, K, squared=True)
    P = nn.joint_p_from_neighbours(idx, d2, perplexity)
    rp, col, val = tsne._affinities_nn(idx, d2, perplexity, squared=True)
    assert np.array_equal(rp, P.indptr) and np.array_equal(col, P.indices)
    np.testing.assert_allclose(val, P.data, rtol=1e-10, atol=0)
    # a row's neighbours in another order: the same structure, values at the same bar
    rng = np.random.default_rng(43)
    perm = np.argsort(rng.random(idx.shape), axis=1)
    pi, pd = np.take_along_axis(idx, perm, 1), np.take_along_axis(d2, perm, 1)
    rp2, col2, val2 = tsne._affinities_nn(pi, pd, perplexity, squared=True)
    assert np.array_equal(rp2, P.indptr) and np.array_equal(col2, P.indices)
    np.testing.assert_allclose(val2, P.data, rtol=1e-10, atol=0)
    # Euclidean distances in, squared on the device: the root and the square cost a few ulp of d2
    rp3, col3, val3 = tsne._affinities_nn(idx, np.sqrt(d2), perplexity)
    assert np.array_equal(rp3, P.indptr) and np.array_equal(col3, P.indices)
    np.testing.assert_allclose(val3, P.data, rtol=1e-10, atol=0)


def _ring_lists(n, K):
    """row i names i + 1 .. i + K mod n, with squared distances that ascend along a row and differ between rows"""
    idx = _snn_ref.ring(n, K)
    d2 = np.sort(np.random.default_rng(n * 1000 + K).uniform(0.5, 2.0, size=(n, K)), axis=1)
    return idx, d2


def _check_p(idx, d2, perplexity):
    """the stage's P against the reference's: the pattern exactly, the values at the bar of test_affinities_from_neighbours_match_reference"""
    from sharp_amd import tsne

    P = nn.joint_p_from_neighbours(idx, d2, perplexity)
    rp, col, val = tsne._affinities_nn(idx, d2, perplexity, squared=True)
    assert np.array_equal(rp, P.indptr) and np.array_equal(col, P.indices)
    np.testing.assert_allclose(val, P.data, rtol=1e-10, atol=0)
    return rp, col


# The edges of the CSR builder behind the symmetrisation (sort by row * n + col, merge equal keys, split the keys) that k-NN lists of
# random points do not pin down.
def test_affinities_without_a_mutual_pair(sa):
    """a directed ring, n = 40, K = 3: i names j and j names i never both (that needs a + b = 0 mod 40 with a, b in 1 .. 3), so no key
    appears twice and nothing is merged"""
    idx, d2 = _ring_lists(40, 3)
    rp, col = _check_p(idx, d2, 2.0)
    assert col.size == 2 * 40 * 3 and np.array_equal(np.diff(rp), np.full(40, 6))


def test_affinities_with_every_pair_mutual(sa):
    """the complete graph, n = K + 1 = 9: every key appears twice"""
    n = 9
    idx = _snn_ref.complete_lists(n)
    d2 = np.sort(np.random.default_rng(9).uniform(0.5, 2.0, size=(n, n - 1)), axis=1)
    rp, col = _check_p(idx, d2, 2.0)
    assert col.size == n * (n - 1) and np.array_equal(col.reshape(n, n - 1), idx)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_affinities_where_the_key_width_changes(sa, n):
    """n * n reaches 2^16 at n = 256, so the sort's end bit (the width of n * n) moves from 16 to 17; the largest key, the last row's
    last column (n - 1, n - 2), must come out last"""
    idx, d2 = _ring_lists(n, 5)
    assert (n * n).bit_length() == (16 if n == 255 else 17)
    rp, col = _check_p(idx, d2, 3.0)
    assert rp[n] == col.size == 2 * n * 5 and rp[n - 1] < rp[n] and col[-1] == n - 2
    assert col[0] == 1 and rp[0] == 0 and rp[1] == 10                # (row 0: the columns 1 .. 5 and n - 5 .. n - 1)


# ---- 3. the bits of the direct path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("repulsion", ["exact", "barnes_hut"])
def test_neighbours_fed_back_give_the_bits_of_the_direct_path(sa, repulsion):
    X = _blobs(1000, 20, 4, 44)
    loop = dict(perplexity=30, seed=7, stop_lying_iter=20, mom_switch_iter=30, max_iter=60, repulsion=repulsion)
    want = sa.Rtsne(X, pca=False, normalize=False, check_duplicates=False, **loop)
    idx, d2 = sa.knn(X, 90, squared=True)
    got = sa.Rtsne_neighbors(idx, d2, squared=True, **loop)
    assert got["itercosts"].shape == (2,) and got["origD"] is None and got["N"] == 1000
    for key in ("Y", "itercosts", "costs"):
        assert np.array_equal(got[key], want[key]), key
    # Euclidean distances (a root and a square in between): the bar of test_tsne_gpu.py's short runs
    Y0 = np.random.default_rng(45).normal(size=(1000, 2)) * 1e-2
    short = dict(perplexity=30, max_iter=10, Y_init=Y0, repulsion=repulsion)
    w10 = sa.Rtsne(X, pca=False, normalize=False, check_duplicates=False, **short)["Y"]
    g10 = sa.Rtsne_neighbors(idx, np.sqrt(d2), **short)["Y"]
    np.testing.assert_allclose(g10, w10, rtol=0, atol=1e-6 * np.abs(w10).max())


# ---- 4. is_distance end to end -----------------------------------------------------------------------------------------------------
def test_is_distance_end_to_end(sa):
    n = 800
    X = _blobs(n, 12, 4, 46)
    d = sa.dist(X, "manhattan")
    D = nn.square_form(d, n)
    Y0 = np.random.default_rng(47).normal(size=(n, 2)) * 1e-2
    out = sa.Rtsne(d, is_distance=True, perplexity=15, Y_init=Y0, max_iter=10)
    idx, dsel = nn.knn_from_dist(D, 45)
    Yr, cr = ref.optimise(nn.joint_p_from_neighbours(idx, dsel * dsel, 15), Y0, max_iter=10, stop_lying_iter=0, mom_switch_iter=0)
    np.testing.assert_allclose(out["Y"], Yr, rtol=0, atol=1e-6 * np.abs(Yr).max())
    np.testing.assert_allclose(out["itercosts"], cr, rtol=1e-5)
    assert out["origD"] is None and out["N"] == n
    om = sa.Rtsne(D, is_distance=True, perplexity=15, Y_init=Y0, max_iter=10)                      # the matrix form
    assert np.array_equal(om["Y"], out["Y"]) and np.array_equal(om["costs"], out["costs"])
    oi = sa.Rtsne(d, is_distance=True, perplexity=15, Y_init=Y0, max_iter=10, pca=True, normalize=True, initial_dims=3,
                  check_duplicates=True)                                                         # ignored for a distance input
    assert np.array_equal(oi["Y"], out["Y"])
    ob = sa.Rtsne(d, is_distance=True, perplexity=15, Y_init=Y0, max_iter=10, repulsion="barnes_hut", theta=0.0)
    assert np.array_equal(ob["Y"], out["Y"])                                                     # theta = 0 is the exact path
    # the same map through the stages: knn on the distances, then Rtsne_neighbors
    ki, kd = sa.knn(d, 45, is_distance=True)
    on = sa.Rtsne_neighbors(ki, kd, perplexity=15, Y_init=Y0, max_iter=10)
    assert np.array_equal(on["Y"], out["Y"])


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_leave_the_library_usable(sa):
    E = sa.SharpError
    n, K = 300, 30
    X = _blobs(n, 6, 3, 48)
    idx, d2 = sa.knn(X, K, squared=True)

    def good():
        assert sa.Rtsne_neighbors(idx, d2, squared=True, perplexity=10, max_iter=2)["Y"].shape == (n, 2)

    def bad_index(row, colm, value, match):
        b = idx.copy()
        b[row, colm] = value
        b[row + 40, 0] = value if value != row else row + 40         # a later row offends too: the first one is named
        with pytest.raises(E, match=match):
            sa.Rtsne_neighbors(b, d2, squared=True, perplexity=10, max_iter=2)
        good()

    bad_index(57, 3, n, r"outside \[0, n\) \(row 57,")
    bad_index(58, 29, -1, r"outside \[0, n\) \(row 58,")
    bad_index(59, 7, 59, r"names itself as a neighbour \(row 59,")
    b = idx.copy()
    b[61, 20] = b[61, 2]
    b[200, 5] = b[200, 4]
    with pytest.raises(E, match=r"twice in a row \(row 61,"):
        sa.Rtsne_neighbors(b, d2, squared=True, perplexity=10, max_iter=2)
    good()
    for v in (np.nan, -1e-3, np.inf):
        bd = d2.copy()
        bd[63, 11] = v
        with pytest.raises(E, match=r"NA / NaN / Inf or negative \(row 63,"):
            sa.Rtsne_neighbors(idx, bd, squared=True, perplexity=10, max_iter=2)
        good()
    # an index and a distance at fault in one row: the index is reported (nothing may dereference it)
    bd = d2.copy()
    bd[10, 0] = np.nan
    b = idx.copy()
    b[10, 1] = 10 ** 6
    with pytest.raises(E, match=r"outside \[0, n\) \(row 10,"):
        sa.Rtsne_neighbors(b, bd, squared=True, perplexity=10, max_iter=2)
    good()
    with pytest.raises(E, match=r"outside \[0, n\) \(row 5,"):     # an index no int32 holds
        big = idx.astype(np.int64)
        big[5, 5] = 2 ** 40
        sa.Rtsne_neighbors(big, d2, squared=True, perplexity=10, max_iter=2)
    good()
    with pytest.raises(E, match="perplexity above K"):
        sa.Rtsne_neighbors(idx, d2, squared=True, perplexity=31, max_iter=2)
    good()
    with pytest.raises(E, match="Perplexity is too large"):
        sa.Rtsne_neighbors(idx[:60, :25] % 60, d2[:60, :25], squared=True, perplexity=20, max_iter=2)
    with pytest.raises(E, match="Incorrect theta"):
        sa.Rtsne_neighbors(idx, d2, squared=True, perplexity=10, max_iter=2, repulsion="barnes_hut", theta=1.5)
    with pytest.raises(E, match="differ in shape"):
        sa.Rtsne_neighbors(idx, d2[:, :-1], squared=True, perplexity=10, max_iter=2)
    with pytest.raises(E, match="at most 255 neighbours"):
        sa.Rtsne_neighbors(np.zeros((n, 256), np.int32), np.ones((n, 256)), perplexity=10, max_iter=2)
    with pytest.raises(E, match="K <= n - 1"):
        sa.Rtsne_neighbors(np.zeros((20, 20), np.int32), np.ones((20, 20)), perplexity=3, max_iter=2)
    good()
    # the C entries refuse K themselves
    L = sa.lib()
    L.sharp_last_error.restype = C.c_char_p
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))           # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))              # noqa: E731
    rp, nnz = np.zeros(n + 1, np.int64), C.c_longlong()
    col, val = np.zeros(2 * n * 256, np.int32), np.zeros(2 * n * 256)
    for KK, nn_, msg in ((256, n, b"at most 255 neighbours per row"), (20, 20, b"K <= n - 1"), (0, n, b"K >= 1")):
        bi, bdist = np.zeros((nn_, max(KK, 1)), np.int32), np.ones((nn_, max(KK, 1)))
        rc = L.sharp_tsne_affinities_nn(ip(bi), dp(bdist), C.c_longlong(nn_), KK, 1, C.c_double(3.0), C.c_longlong(col.size),
                                        rp.ctypes.data_as(C.POINTER(C.c_longlong)), ip(col), dp(val), C.byref(nnz))
        assert rc != 0 and msg in L.sharp_last_error()
    good()
    # distance input
    d = sa.dist(X, "euclidean")
    for v, match in ((-1.0, "negative value"), (np.nan, "negative value")):
        bd = d.copy()
        bd[1234] = v
        with pytest.raises(E, match=match):
            sa.Rtsne(bd, is_distance=True, perplexity=10, max_iter=2)
        rc = L.sharp_tsne_knn_dist(dp(bd), n, K, ip(np.zeros((n, K), np.int32)), dp(np.zeros((n, K))))
        assert rc != 0 and b"NA / NaN / Inf or a negative distance" in L.sharp_last_error()
    with pytest.raises(E, match="no such length"):
        sa.Rtsne(d[:-1], is_distance=True, perplexity=10, max_iter=2)
    with pytest.raises(E, match="above 85"):
        sa.Rtsne(d, is_distance=True, perplexity=86, max_iter=2)
    with pytest.raises(E, match="Perplexity is too large"):
        sa.Rtsne(sa.dist(X[:50], "euclidean"), is_distance=True, perplexity=20, max_iter=2)
    assert sa.Rtsne(d, is_distance=True, perplexity=10, max_iter=2)["Y"].shape == (n, 2)
    # n beyond the limit is refused before d is read: a one-element buffer must do
    one = np.zeros(1)
    Y = np.zeros((4, 2))
    rc = L.sharp_tsne_dist(dp(one), 46341, 0, 2, C.c_double(30.0), C.c_double(0.5), 2, 0, 0, C.c_double(0.5), C.c_double(0.8),
                           C.c_double(200.0), C.c_double(12.0), None, C.c_double(1.0), dp(Y), None, None)
    assert rc != 0 and b"46340" in L.sharp_last_error()
    rc = L.sharp_tsne_knn_dist(dp(one), 46341, 30, ip(np.zeros(4, np.int32)), dp(np.zeros(4)))
    assert rc != 0 and b"46340" in L.sharp_last_error()
    good()


# ---- 6. visualization_SHARP --------------------------------------------------------------------------------------------------------
def test_visualization_sharp_returns_and_reuses_neighbours(sa, oracle):
    X = oracle.synth_fill(20261003, 1500, 0, 1200, 4, 200)
    res = sa.SHARP(X, rN_seed=2103, ensize_K=3)
    L = sa.lib()

    def knn_launches():
        ms, cnt = C.c_double(), C.c_longlong(-1)
        assert L.sharp_profile_get(b"tsne_knn", C.byref(ms), C.byref(cnt)) == 0
        return cnt.value

    v0 = sa.visualization_SHARP(res, plot=False, max_iter=60)
    assert "neighbors" not in v0
    L.sharp_profile_enable(1)
    try:
        L.sharp_profile_reset()
        v1 = sa.visualization_SHARP(res, plot=False, max_iter=60, return_neighbors=True)
        assert knn_launches() >= 1                                   # (the counter sees the k-NN when it runs)
        assert np.array_equal(v1["Y"], v0["Y"]) and np.array_equal(v1["itercosts"], v0["itercosts"])
        nb = v1["neighbors"]
        assert set(nb) == {"index", "distance", "squared", "w", "n"} and nb["squared"] is True and nb["n"] == 1200 and nb["w"] == 2
        assert nb["index"].shape == (1200, 90) and nb["index"].dtype == np.int32
        L.sharp_profile_reset()
        v2 = sa.visualization_SHARP(res, plot=False, max_iter=60, neighbors=nb, seed=3)
        assert knn_launches() == 0
        v3 = sa.visualization_SHARP(res, plot=False, max_iter=60, neighbors=nb, return_neighbors=True)
        assert knn_launches() == 0
    finally:
        L.sharp_profile_enable(0)
    assert v2["Y"].shape == (1200, 2) and not np.array_equal(v2["Y"], v0["Y"]) and "neighbors" not in v2
    assert np.array_equal(v3["Y"], v0["Y"]) and v3["neighbors"] is nb
    # a smaller perplexity takes the lists' first columns: what Rtsne computes itself
    v4 = sa.visualization_SHARP(res, plot=False, max_iter=20, neighbors=nb, perplexity=10)
    assert np.array_equal(v4["Y"], sa.visualization_SHARP(res, plot=False, max_iter=20, perplexity=10)["Y"])
    with pytest.raises(sa.SharpError, match="computed with w = 2"):
        sa.visualization_SHARP(res, w=3, plot=False, max_iter=20, neighbors=nb)
    with pytest.raises(sa.SharpError, match="computed for 1000 cells"):
        sa.visualization_SHARP(res, plot=False, max_iter=20, neighbors=dict(nb, n=1000))
    with pytest.raises(sa.SharpError, match="needs 120 neighbours"):
        sa.visualization_SHARP(res, plot=False, max_iter=20, neighbors=nb, perplexity=40)


# ---- 7. the .C() twins and the R glue ----------------------------------------------------------------------------------------------
def test_dotc_twins(sa):
    """the .C() convention (tests/test_dotc_gpu.py): same outputs as the C entries, status set on a refusal"""
    L = sa.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    I = lambda v: np.array([v], np.int32)                            # noqa: E731
    D = lambda v: np.array([v], np.float64)                          # noqa: E731
    for f in ("sharp_C_tsne_neighbors", "sharp_C_tsne_dist", "sharp_C_tsne_knn", "sharp_C_last_error"):
        getattr(L, f).restype = None
    n, K = 600, 45
    X = np.ascontiguousarray(_blobs(n, 10, 3, 22))
    Y0 = np.random.default_rng(23).normal(size=(n, 2)) * 1e-2
    idx, d2, st = np.zeros((n, K), np.int32), np.zeros((n, K)), I(-1)
    L.sharp_C_tsne_knn(P(X), P(D(n)), P(I(10)), P(I(K)), P(idx), P(d2), P(st))
    ri, rd = sa.knn(X, K, squared=True)
    assert st[0] == 0 and np.array_equal(idx, ri) and np.array_equal(d2, rd)
    for rep, name in ((0, "exact"), (1, "barnes_hut")):
        Y, ic, costs = np.zeros((n, 2)), np.zeros(2), np.zeros(n)
        tail = [I(rep), I(2), D(15.0), D(0.5), I(60), I(0), I(0), D(0.5), D(0.8), D(200.0), D(12.0), I(1), Y0, D(10.0), Y, ic, costs, st]
        st[0] = -1
        L.sharp_C_tsne_neighbors(*[P(a) for a in [idx, d2, D(n), I(K), I(1)] + tail])
        want = sa.Rtsne_neighbors(idx, d2, squared=True, perplexity=15, max_iter=60, Y_init=Y0, repulsion=name)
        assert st[0] == 0 and np.array_equal(Y, want["Y"]) and np.array_equal(ic, want["itercosts"]) and np.array_equal(costs, want["costs"])
        d = sa.dist(X, "maximum")
        Y[:], ic[:], costs[:], st[0] = 0, 0, 0, -1
        L.sharp_C_tsne_dist(*[P(a) for a in [d, I(n)] + tail])
        want = sa.Rtsne(d, is_distance=True, perplexity=15, max_iter=60, Y_init=Y0, repulsion=name)
        assert st[0] == 0 and np.array_equal(Y, want["Y"]) and np.array_equal(ic, want["itercosts"]) and np.array_equal(costs, want["costs"])
    # has_Y_init = 0: the start comes from the seed
    tail[11] = I(0)
    L.sharp_C_tsne_neighbors(*[P(a) for a in [idx, d2, D(n), I(K), I(1)] + tail])
    assert st[0] == 0
    assert np.array_equal(Y, sa.Rtsne_neighbors(idx, d2, squared=True, perplexity=15, max_iter=60, seed=10, stop_lying_iter=0,
                                                mom_switch_iter=0, repulsion="barnes_hut")["Y"])
    # refusals: the status and the message
    buf = C.create_string_buffer(b" " * 255)
    msg, ln = (C.c_char_p * 1)(C.addressof(buf)), (C.c_int * 1)(256)
    bad = idx.copy()
    bad[17, 4] = n
    L.sharp_C_tsne_neighbors(*[P(a) for a in [bad, d2, D(n), I(K), I(1)] + tail])
    L.sharp_C_last_error(msg, ln)
    assert st[0] != 0 and b"outside [0, n) (row 17," in buf.value
    tail[2] = D(300.0)
    L.sharp_C_tsne_dist(*[P(a) for a in [d, I(n)] + tail])
    assert st[0] != 0
    L.sharp_C_tsne_knn(P(X), P(D(n)), P(I(10)), P(I(256)), P(idx), P(d2), P(st))
    assert st[0] != 0


def test_r_glue_takes_one_based_indices(sa):
    """r/sharp_glue.c's .Call entries behind sharp_Rtsne_neighbors and sharp_Rtsne(is_distance = TRUE), run against tests/rmock as
    tests/test_rglue_gpu.py does: R-shaped values in (an integer matrix of 1-based indices, numeric matrices, a dist vector), R's list out"""
    from _rglue import Glue

    g = Glue()
    g.call("R_sharp_init", g.int(0))
    n, K = 500, 30
    X = _blobs(n, 8, 3, 49)
    Y0 = np.random.default_rng(50).normal(size=(n, 2)) * 1e-2
    idx, dist = sa.knn(X, K)
    want = sa.Rtsne_neighbors(idx, dist, perplexity=10, max_iter=60, Y_init=Y0, repulsion="barnes_hut", theta=0.4)
    ipar = g.int(0, 1, 2, 60, 0, 0)
    dpar = g.real(10.0, 0.4, 0.5, 0.8, 200.0, 12.0, 10.0)
    r = g.call("R_sharp_tsne_neighbors", g.int(np.asfortranarray(idx + 1).ravel(order="F")), g.matrix(dist), ipar, dpar, g.matrix(Y0))
    assert np.array_equal(g.get(r, "Y"), want["Y"]) and np.array_equal(g.get(r, "itercosts"), want["itercosts"])
    assert np.array_equal(g.get(r, "costs"), want["costs"])
    # no Y_init: numeric(0); the start comes from the seed
    w2 = sa.Rtsne_neighbors(idx, dist, perplexity=10, max_iter=60, seed=4)
    r = g.call("R_sharp_tsne_neighbors", g.int(np.asfortranarray(idx + 1).ravel(order="F")), g.matrix(dist), g.int(0, 0, 2, 60, 250, 250),
               g.real(10.0, 0.5, 0.5, 0.8, 200.0, 12.0, 4.0), g.real())
    assert np.array_equal(g.get(r, "Y"), w2["Y"])
    # index 0 is R's "no such row": refused with the row's name, as an R error
    b = idx + 1
    b[33, 2] = 0
    with pytest.raises(RuntimeError, match=r"outside \[0, n\) \(row 33,"):
        g.call("R_sharp_tsne_neighbors", g.int(np.asfortranarray(b).ravel(order="F")), g.matrix(dist), ipar, dpar, g.matrix(Y0))
    d = sa.dist(X, "manhattan")
    wd = sa.Rtsne(d, is_distance=True, perplexity=10, max_iter=60, Y_init=Y0)
    r = g.call("R_sharp_tsne_dist", g.real(d), g.int(n), g.int(0, 0, 2, 60, 0, 0), dpar, g.matrix(Y0))
    assert np.array_equal(g.get(r, "Y"), wd["Y"]) and np.array_equal(g.get(r, "costs"), wd["costs"])
    with pytest.raises(RuntimeError, match="n \\(n - 1\\) / 2"):
        g.call("R_sharp_tsne_dist", g.real(d[:-1]), g.int(n), g.int(0, 0, 2, 60, 0, 0), dpar, g.matrix(Y0))
    g.reset()
