"""GPU tests of sharp_dist / sharp_hclust_dist / sharp_hclust: R's dist vector and R's hclust object (merge, height,
order) against numpy loops of the same formulas and against hclust.f's HCASS2 applied to the oracle's agglomeration."""
import ctypes as C

import numpy as np
import pytest

from _tree_ref import hcass2

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
METHODS = ["ward.D", "single", "complete", "average", "mcquitty", "median", "centroid", "ward.D2"]


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


def _tri(n):
    """pairs (i > j) in R's dist order: column-wise lower triangle"""
    j, i = np.triu_indices(n, 1)
    return i, j


def _dist_loop(x, method, p=2.0):
    """fp64 loop over the features in the order k = 0 .. p - 1, from the differences"""
    i, j = _tri(x.shape[0])
    acc = np.zeros(i.size)
    for k in range(x.shape[1]):
        d = x[i, k] - x[j, k]
        if method == "euclidean":
            acc = acc + d * d
        elif method == "manhattan":
            acc = acc + np.abs(d)
        elif method == "maximum":
            acc = np.maximum(acc, np.abs(d))
        else:
            acc = acc + np.abs(d) ** p
    return np.sqrt(acc) if method == "euclidean" else acc ** (1.0 / p) if method == "minkowski" else acc


@pytest.mark.parametrize("method", ["euclidean", "manhattan", "maximum", "minkowski"])
def test_dist_difference_methods(sa, method):
    """Tolerance, derived: p non-negative terms summed in any order plus one root are within (p + 3) 2^-53 relative.  minkowski: every
    pow() call (one per term, one at the end; device pow is within 4 ulp = 8 half-ulps, numpy's within 1 ulp = 2) adds its own."""
    n, p = 1025, 37                                          # not a multiple of the 64 x 64 tile, nor of the 32-feature pass
    rng = np.random.default_rng(11)
    x = rng.normal(size=(n, p))
    x[700] = x[3]                                            # exact copies
    x[1024] = x[3]
    got = sa.dist(x, method=method, p=3)
    ref = _dist_loop(x, method, 3.0)
    tol = (p + 3) * EPS + (2 * (8 + 2) * EPS if method == "minkowski" else 0.0)
    err = np.abs(got - ref) / np.maximum(ref, 1e-300)
    print(method, "max relative error", err[ref > 0].max(), "bound", tol)
    assert got.shape == ref.shape and np.all(err[ref > 0] <= tol)
    i, j = _tri(n)
    dup = (np.isin(i, [3, 700, 1024])) & (np.isin(j, [3, 700, 1024]))
    assert dup.sum() == 3 and np.all(got[dup] == 0.0) and np.all(got[~dup] > 0)
    full = np.zeros((n, n))
    full[i, j] = got
    full[j, i] = got
    assert np.array_equal(full[3], full[700]) and np.array_equal(full[3], full[1024])   # copies: bitwise-equal distances to every row


def test_dist_correlation_and_refusals(sa, oracle):
    n, p = 1025, 37
    x = np.random.default_rng(12).normal(size=(n, p))
    got = sa.dist(x, method="correlation")
    np.testing.assert_allclose(got, oracle.cor_dist(x), rtol=0, atol=1e-13 * p)          # tests/test_linalg_gpu.py's bound for that GEMM
    for m in ("canberra", "binary"):
        with pytest.raises(sa.SharpError, match="not supported"):
            sa.dist(x, method=m)
    with pytest.raises(sa.SharpError, match="invalid distance"):
        sa.dist(x, method="cosine")
    x[5, 5] = np.nan
    with pytest.raises(sa.SharpError, match="NA / NaN / Inf"):
        sa.dist(x)
    L = sa.lib()
    L.sharp_last_error.restype = C.c_char_p
    out = np.zeros(1)
    rc = L.sharp_dist(x.ctypes.data_as(C.POINTER(C.c_double)), 2, 3, C.c_longlong(37), 5, C.c_double(2.0), out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc != 0 and b"not supported" in L.sharp_last_error()


def _check_tree(tree, ia, ib, crit):
    merge, order = hcass2(ia, ib)
    assert np.array_equal(tree["merge"], merge)
    assert np.array_equal(tree["order"], order)
    np.testing.assert_allclose(tree["height"], crit, rtol=1e-9, atol=1e-12)              # tests/test_hclust_gpu.py::_compare


@pytest.mark.parametrize("n", [41, 700, 4097])
@pytest.mark.parametrize("method", METHODS)
def test_hclust_from_distances_matches_r_object(sa, oracle, method, n):
    d = np.random.default_rng(100 + n).random(n * (n - 1) // 2) + 0.5                    # continuous: no two distances equal
    tree = sa.hclust(d=d, method=method)
    assert tree["n"] == n and tree["method"] == method
    _check_tree(tree, *oracle.hclust(d, n, method))


@pytest.mark.parametrize("method", ["ward.D", "average", "single"])
def test_hclust_with_exact_ties_follows_r_order(sa, oracle, method):
    """5 % of the rows duplicated: exact zeros and exactly equal pairs in the distance vector; the sequential kernel (R's order) must run"""
    n = 3000
    rng = np.random.default_rng(5)
    x = rng.normal(size=(n, 20))
    src = rng.choice(n, n // 20, replace=False)
    dst = rng.choice(np.setdiff1d(np.arange(n), src), n // 20, replace=False)
    x[dst] = x[src]
    d = sa.dist(x)
    assert np.count_nonzero(d == 0.0) >= n // 20
    L = sa.lib()
    L.sharp_profile_enable(1)
    L.sharp_profile_reset()
    tree = sa.hclust(d=d, method=method)
    ms, k = C.c_double(), C.c_longlong()
    L.sharp_profile_get(b"host:hclust_tasks_sequential", C.byref(ms), C.byref(k))
    L.sharp_profile_enable(0)
    assert k.value == 1
    _check_tree(tree, *oracle.hclust(d, n, method))


@pytest.mark.parametrize("distance", ["euclidean", "correlation"])
@pytest.mark.parametrize("n", [2000, 10040])
def test_fused_hclust_equals_hclust_of_dist(sa, distance, n):
    x = np.random.default_rng(n).normal(size=(n, 30))
    a = sa.hclust(x=x, distance=distance)
    b = sa.hclust(d=sa.dist(x, method=distance))
    assert a["dist_method"] == distance
    for key in ("merge", "order", "height"):
        assert np.array_equal(a[key], b[key]), key


def test_fused_hclust_at_the_size_limit(sa):
    n = 16384
    x = np.random.default_rng(1).normal(size=(n, 16))
    t = sa.hclust(x=x)
    assert np.array_equal(np.sort(t["order"]), np.arange(1, n + 1))
    assert np.all(np.diff(t["height"]) >= 0) and t["merge"].min() == -n and t["merge"].max() == n - 2
    assert np.array_equal(np.sort(-t["merge"][t["merge"] < 0]), np.arange(1, n + 1))
    with pytest.raises(sa.SharpError, match="more than 16384"):
        sa.hclust(x=np.zeros((n + 1, 2)))
    t2 = sa.hclust(x=np.array([[0.0, 0.0], [3.0, 4.0]]))
    assert t2["merge"].tolist() == [[-1, -2]] and t2["height"].tolist() == [5.0] and t2["order"].tolist() == [1, 2]
    t3 = sa.hclust(d=[5.0])
    assert t3["merge"].tolist() == [[-1, -2]] and t3["height"].tolist() == [5.0] and t3["order"].tolist() == [1, 2]
    with pytest.raises(sa.SharpError, match="more than 46340"):
        sa.dist(np.zeros((46341, 1)))


def test_dotc_twins(sa, oracle):
    """the .C() convention (tests/test_dotc_gpu.py): same outputs as the C entries, status set on a refusal"""
    L = sa.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)                                           # noqa: E731
    I = lambda *v: np.array(v, np.int32)                                                 # noqa: E731
    n, p = 300, 9
    x = np.random.default_rng(3).normal(size=(n, p))
    d, st = np.zeros(n * (n - 1) // 2), I(-1)
    for f in ("sharp_C_dist", "sharp_C_hclust_dist", "sharp_C_hclust"):
        getattr(L, f).restype = None
    L.sharp_C_dist(P(x), P(I(n)), P(I(p)), P(I(1)), P(np.array([2.0])), P(d), P(st))
    assert st[0] == 0 and np.array_equal(d, sa.dist(x))
    ref = sa.hclust(d=d, method="average")
    for fused in (False, True):
        merge, height, order = np.zeros(2 * (n - 1), np.int32), np.zeros(n - 1), np.zeros(n, np.int32)
        if fused:
            L.sharp_C_hclust(P(x), P(I(n)), P(I(p)), P(I(1)), P(np.array([2.0])), P(I(4)), P(merge), P(height), P(order), P(st))
        else:
            L.sharp_C_hclust_dist(P(d), P(I(n)), P(I(4)), P(merge), P(height), P(order), P(st))
        assert st[0] == 0
        assert np.array_equal(merge.reshape(2, n - 1).T, ref["merge"]) and np.array_equal(order, ref["order"])
        assert np.array_equal(height, ref["height"])
    L.sharp_C_dist(P(x), P(I(n)), P(I(p)), P(I(4)), P(np.array([2.0])), P(d), P(st))
    assert st[0] != 0
    L.sharp_C_hclust_dist(P(d), P(I(n)), P(I(9)), P(merge), P(height), P(order), P(st))
    assert st[0] != 0


def test_c_abi_with_a_leading_dimension(sa):
    """observations held in a wider array (ld > p): the same dist vector and tree as from the packed copy"""
    L = sa.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                               # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))                                  # noqa: E731
    n, p, ld = 333, 21, 29
    wide = np.random.default_rng(9).normal(size=(n, ld))
    x = np.ascontiguousarray(wide[:, :p])
    d = np.zeros(n * (n - 1) // 2)
    assert L.sharp_dist(dp(wide), n, p, C.c_longlong(ld), 3, C.c_double(2.0), dp(d)) == 0
    assert np.array_equal(d, sa.dist(x, method="manhattan"))
    merge, height, order = np.zeros((2, n - 1), np.int32), np.zeros(n - 1), np.zeros(n, np.int32)
    assert L.sharp_hclust(dp(wide), n, p, C.c_longlong(ld), 1, C.c_double(2.0), 3, ip(merge), dp(height), ip(order)) == 0
    ref = sa.hclust(x=x, method="complete")
    assert np.array_equal(merge.T, ref["merge"]) and np.array_equal(order, ref["order"]) and np.array_equal(height, ref["height"])
