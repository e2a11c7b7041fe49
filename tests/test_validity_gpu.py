"""GPU tests of silhouette() / calinski_harabasz() / cutree() against numpy restatements of sildist(), the oracle, scipy and
sklearn -- never against another path of the library.

Tolerance of a silhouette width, derived: a per-cluster mean of at most n non-negative distances, each within (p + 3) 2^-53 relative
(tests/test_tree_gpu.py's bound for a distance), summed in any order, is within e = (n + p + 4) 2^-53 relative.  In w = (b - a) / M,
M = max(a, b), the numerator moves by at most e (a + b) <= 2 e M and the denominator by e M with |w| <= 1: w is within 3 e plus two
roundings.  Both sides carry that error: 6 (n + p + 5) 2^-53.  minkowski adds the pow() terms tests/test_tree_gpu.py adds to a distance
(2 (8 + 2) half-ulps); correlation adds the distance GEMM's existing bound of 1e-13 p per distance over the smallest mean distance of the
input, computed from the reference."""
import ctypes as C
import time

import numpy as np
import pytest

from _validity_ref import (EPS, SCIPY_METRIC, cdist_rows, ch_euclid, exact_case, gaussian_clusters, recode, sildist, sildist_full,
                           squareform_rows)

pytestmark = pytest.mark.gpu

DISTANCES = ["euclidean", "maximum", "manhattan", "minkowski", "correlation"]


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


def _tol(n, p, distance="euclidean", min_mean=None):
    t = 6 * (n + p + 5) * EPS
    if distance == "minkowski":
        t += 6 * 2 * (8 + 2) * EPS
    if distance == "correlation":
        t += 1e-13 * p / min_mean
    return t


def _min_mean(ref):
    return min(ref["a"][ref["a"] > 0].min(), ref["b"].min())


def _check(res, ref_width, ref, labels, levels, n, p, distance, what):
    """widths within the derived bound; neighbours equal for EVERY cell, which is fair because the reference decides each by a margin
    far above the arithmetic (asserted)"""
    assert ref["gap"].min() > 1e-9, (what, ref["gap"].min())
    tol = _tol(n, p, distance, _min_mean(ref))
    err = np.abs(res["sil_width"] - ref_width).max()
    print(what, "max |width - reference|", err, "bound", tol, "smallest neighbour gap", ref["gap"].min())
    assert err <= tol, (what, err, tol)
    assert np.array_equal(res["neighbor"], levels[ref["neighbor"] - 1]), what
    assert np.array_equal(res["cluster"], labels)


def test_exact_arithmetic_case_is_bitwise(sa):
    """integer data under manhattan: every distance and per-cluster sum is an exact integer below 2^53, so no order of summation can
    matter and the result must be sildist()'s bit for bit, ties included"""
    from scipy.spatial.distance import pdist

    x, labels, u = exact_case()
    cl, levels = recode(labels)
    k = levels.size
    assert x.shape == (490, 6) and k == 6 and not np.array_equal(levels, np.arange(1, 7))
    ref = sildist(cdist_rows(x, "manhattan"), cl, k)
    # the input exercises the tie rules
    tie = ref["gap"] == 0.0
    assert tie.sum() >= 50                                     # two equal smallest means: the copy cluster
    assert set(levels[ref["neighbor"][tie] - 1].tolist()) == {3}           # ... decided for the first in sorted label order (3 before 11)
    assert ref["a"][u] == ref["b"][u] == 1.0 and labels[u] == 40 and levels[ref["neighbor"][u] - 1] == -7     # a == b
    assert np.count_nonzero(ref["a"] == ref["b"]) == 1 and np.count_nonzero(ref["width"] == 0.0) == 2         # u and the singleton w
    o = np.random.default_rng(1).permutation(490)              # the restatement itself does not depend on the order of the cells
    ref2 = sildist(cdist_rows(x[o], "manhattan"), cl[o], k)
    assert np.array_equal(ref2["width"], ref["width"][o]) and np.array_equal(ref2["neighbor"], ref["neighbor"][o])
    d = pdist(x, "cityblock")
    for name, res in (("data=", sa.silhouette(labels, data=x, distance="manhattan")), ("d=", sa.silhouette(labels, d=d))):
        assert np.array_equal(res["sil_width"], ref["width"]), name
        assert np.array_equal(res["neighbor"], levels[ref["neighbor"] - 1]), name
        assert np.array_equal(res["cluster"], labels), name
        assert np.array_equal(res["clus_sizes"], np.bincount(cl - 1)), name
        assert res["clus_avg_widths"].shape == (6,) and abs(res["avg_width"] - ref["width"].mean()) < 1e-15, name
    res = sa.silhouette({"pred_clusters": labels}, data=x[:, :6], distance="manhattan")      # a SHARP* result dict
    assert np.array_equal(res["sil_width"], ref["width"])


@pytest.mark.parametrize("distance", DISTANCES)
def test_continuous_case_small_all_distances(sa, oracle, distance):
    """(3001, 37, 8): neither a multiple of the 64-cell tile nor of the 32-feature pass.  Widths against the oracle's silhouette_widths
    on scipy's pdist / the oracle's cor_dist, through data= and through d="""
    from scipy.spatial.distance import pdist

    n, p, g = 3001, 37, 7
    x, labels = gaussian_clusters(21, n, p, g)
    cl, levels = recode(labels)
    k = levels.size
    assert k == g + 1 and np.count_nonzero(labels == g + 1) == 1
    if distance == "correlation":
        dref = oracle.cor_dist(x)
    else:
        dref = pdist(x, SCIPY_METRIC[distance], **({"p": 3.0} if distance == "minkowski" else {}))
    wref = oracle.silhouette_widths(cl, dref)
    ref = sildist(squareform_rows(dref, n), cl, k)              # neighbours and the margins (the oracle returns widths only)
    assert np.abs(ref["width"] - wref).max() <= _tol(n, p)
    r1 = sa.silhouette(labels, data=x, distance=distance, p=3)
    _check(r1, wref, ref, labels, levels, n, p, distance, f"{distance} data=")
    r2 = sa.silhouette(labels, d=dref)                         # (the reference's own distances: only the reduction differs)
    _check(r2, wref, ref, labels, levels, n, p, "euclidean", f"{distance} d=")
    assert r1["sil_width"][n // 2] == 0.0 and r2["sil_width"][n // 2] == 0.0    # the singleton


def test_continuous_case_large_and_determinism(sa):
    """(20011, 50, 13) through data=: euclidean against the restatement and sklearn's silhouette_samples, correlation against
    1 - numpy.corrcoef; two calls give the same bits; d= agrees with data= within the bound"""
    from sklearn.metrics import silhouette_samples

    n, p, g = 20011, 50, 12
    x, labels = gaussian_clusters(22, n, p, g)
    cl, levels = recode(labels)
    k = levels.size
    t0 = time.time()
    ref = sildist(cdist_rows(x, "euclidean"), cl, k)
    sk = silhouette_samples(x, labels)
    print("references took", time.time() - t0, "s; restatement vs sklearn", np.abs(sk - ref["width"]).max())
    assert np.abs(sk - ref["width"]).max() <= _tol(n, p)
    r1 = sa.silhouette(labels, data=x)
    _check(r1, ref["width"], ref, labels, levels, n, p, "euclidean", "euclidean 20011 vs restatement")
    _check(r1, sk, ref, labels, levels, n, p, "euclidean", "euclidean 20011 vs sklearn")
    r2 = sa.silhouette(labels, data=x)
    assert np.array_equal(r1["sil_width"], r2["sil_width"]) and np.array_equal(r1["neighbor"], r2["neighbor"])     # bitwise
    r3 = sa.silhouette(labels, d=sa.dist(x))
    r4 = sa.silhouette(labels, d=sa.dist(x))
    assert np.array_equal(r3["sil_width"], r4["sil_width"])
    err = np.abs(r3["sil_width"] - r1["sil_width"]).max()
    print("d= vs data=", err)
    assert err <= _tol(n, p) and np.array_equal(r3["neighbor"], r1["neighbor"])
    D = np.corrcoef(x)
    np.subtract(1.0, D, out=D)
    np.fill_diagonal(D, 0.0)
    refc = sildist_full(D, cl, k)
    del D
    rc = sa.silhouette(labels, data=x, distance="correlation")
    _check(rc, refc["width"], refc, labels, levels, n, p, "correlation", "correlation 20011")
    rc2 = sa.silhouette(labels, data=x, distance="correlation")
    assert np.array_equal(rc["sil_width"], rc2["sil_width"])


def test_large_n_matrix_free_sample(sa):
    """n = 200003: no n x n matrix exists anywhere; 512 sample cells are checked against their distances to all cells on the CPU"""
    from scipy.spatial.distance import cdist

    n, p, g = 200003, 50, 9
    x, labels = gaussian_clusters(23, n, p, g)
    cl, levels = recode(labels)
    k = levels.size
    sample = np.random.default_rng(7).choice(n, 512, replace=False)
    Ds = cdist(x[sample], x)
    Ds[np.arange(512), sample] = 0.0
    # sildist() for the sample rows only
    counts = np.bincount(cl - 1, minlength=k).astype(np.float64)
    onehot = np.zeros((n, k))
    onehot[np.arange(n), cl - 1] = 1.0
    S = Ds @ onehot
    ci = cl[sample] - 1
    r = np.arange(512)
    den = np.broadcast_to(counts, S.shape).copy()
    den[r, ci] -= 1.0
    single = den[r, ci] == 0
    den[r[single], ci[single]] = 1.0
    m = S / den
    a = m[r, ci].copy()
    m[r, ci] = np.inf
    j = np.argmin(m, 1)
    b = m[r, j]
    m[r, j] = np.inf
    gap = (m.min(1) - b) / b
    w = np.where(single | (a == b), 0.0, (b - a) / np.maximum(a, b))
    assert gap.min() > 1e-9
    res = sa.silhouette(labels, data=x)
    err = np.abs(res["sil_width"][sample] - w).max()
    print("n = 200003 sample: max |width - reference|", err, "bound", _tol(n, p), "smallest gap", gap.min())
    assert err <= _tol(n, p)
    assert np.array_equal(res["neighbor"][sample], levels[j])
    assert res["sil_width"][n // 2] == 0.0 and np.all(np.abs(res["sil_width"]) <= 1.0)
    with pytest.raises(sa.SharpError, match="data="):
        sa.silhouette(np.zeros(46341, np.int64), d=np.broadcast_to(np.float64(1.0), (46341 * 46340 // 2,)))


def test_degenerate_inputs(sa):
    rng = np.random.default_rng(3)
    n = 50
    x = rng.normal(size=(n, 5))
    assert sa.silhouette(np.ones(n, np.int64), data=x) is None                     # k = 1
    assert sa.silhouette(np.arange(n), data=x) is None                             # k = n
    lab = np.arange(n)
    lab[1] = 0                                                                     # k = n - 1
    res = sa.silhouette(lab, data=x)
    ref = sildist(cdist_rows(x, "euclidean"), *recode(lab)[:1], n - 1)
    assert np.abs(res["sil_width"] - ref["width"]).max() <= _tol(n, 5) and np.count_nonzero(res["sil_width"]) == 2
    assert np.array_equal(res["neighbor"], recode(lab)[1][ref["neighbor"] - 1])
    lab3 = np.array([-3, 0, 40])[rng.integers(0, 3, n)]
    res = sa.silhouette(lab3, data=x)
    cl, levels = recode(lab3)
    ref = sildist(cdist_rows(x, "euclidean"), cl, 3)
    assert levels.tolist() == [-3, 0, 40] and np.array_equal(res["cluster"], lab3)
    assert set(res["neighbor"].tolist()) <= {-3, 0, 40} and np.array_equal(res["neighbor"], levels[ref["neighbor"] - 1])
    assert np.abs(res["sil_width"] - ref["width"]).max() <= _tol(n, 5)
    assert np.array_equal(res["sil_width"], sa.silhouette(lab3.astype(np.float64), data=x)["sil_width"])      # whole numbers as doubles
    L = sa.lib()
    L.sharp_profile_enable(1)
    L.sharp_profile_reset()
    with pytest.raises(sa.SharpError, match="'x' must only have integer codes"):
        sa.silhouette(lab3 + 0.25, data=x)
    with pytest.raises(sa.SharpError, match="number of labels"):
        sa.silhouette(lab3[:-1], data=x)
    with pytest.raises(sa.SharpError, match="incompatible"):
        sa.silhouette(lab3[:-1], d=np.ones(n * (n - 1) // 2))
    bad = x.copy()
    bad[7, 2] = np.inf
    with pytest.raises(sa.SharpError, match="NA / NaN / Inf"):
        sa.silhouette(lab3, data=bad)
    with pytest.raises(sa.SharpError, match="NA / NaN / Inf"):
        sa.calinski_harabasz(bad, lab3)
    for m in ("canberra", "binary"):
        with pytest.raises(sa.SharpError, match="not supported"):
            sa.silhouette(lab3, data=x, distance=m)
    ms, cnt = C.c_double(), C.c_longlong()
    for name in (b"silhouette_tiles", b"silhouette_dist", b"ch_within"):          # each refusal came before any kernel ran
        L.sharp_profile_get(name, C.byref(ms), C.byref(cnt))
        assert cnt.value == 0, name
    L.sharp_profile_enable(0)
    # the C entry refuses what the Python layer never passes on
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                         # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))                            # noqa: E731
    L.sharp_last_error.restype = C.c_char_p
    nb, w = np.zeros(n, np.int32), np.zeros(n)
    codes = np.ascontiguousarray(cl, np.int32)
    assert L.sharp_silhouette(dp(x), C.c_longlong(n), 5, C.c_longlong(5), 1, C.c_double(2.0), ip(codes), 4, ip(nb), dp(w)) != 0
    assert b"every cluster code" in L.sharp_last_error()
    assert L.sharp_silhouette(dp(x), C.c_longlong(n), 5, C.c_longlong(5), 1, C.c_double(2.0), ip(codes), 2, ip(nb), dp(w)) != 0
    assert b"between 1 and k" in L.sharp_last_error()
    assert L.sharp_silhouette(dp(x), C.c_longlong(1 << 25), 5, C.c_longlong(5), 1, C.c_double(2.0), ip(codes), 3, ip(nb), dp(w)) != 0
    assert b"16777216" in L.sharp_last_error()


@pytest.mark.parametrize("shape", [(21, 3001, 37, 7), (22, 20011, 50, 12)])
def test_calinski_harabasz(sa, oracle, shape):
    """Euclidean: relative 4 n p 2^-53 (B and W are sums of n p non-negative products over centroids that are themselves sums of at
    most n terms).  1-corr: every 1 - r carries up to (p + 3) 2^-52 absolute and is then squared, so the same bound over the smallest
    1 - r the reference meets."""
    from sklearn.metrics import calinski_harabasz_score

    seed, n, p, g = shape
    x, labels = gaussian_clusters(seed, n, p, g)
    cl, levels = recode(labels)
    k = levels.size
    got = sa.calinski_harabasz(x, labels)
    ref = calinski_harabasz_score(x, labels)
    tol = 4 * n * p * EPS
    print("CH euclidean", got, "sklearn", ref, "relative", abs(got - ref) / ref, "bound", tol, "restatement", ch_euclid(x, cl, k))
    assert abs(got - ref) <= tol * ref
    assert abs(got - ch_euclid(x, cl, k)) <= tol * ref
    got1 = sa.calinski_harabasz(x, labels, distance="1-corr")
    ref1 = oracle.get_CH_1corr(x, cl.astype(np.int32))
    cen = np.stack([x[cl == c].mean(0) for c in range(1, k + 1)])
    unit = lambda a: (a - a.mean(-1, keepdims=True)) / np.linalg.norm(a - a.mean(-1, keepdims=True), axis=-1, keepdims=True)   # noqa: E731
    # (a cell alone in its cluster IS its centroid: its 1 - r is 0 by construction and its term at most ((p + 3) 2^-52)^2 absolute;
    # it is left out of the minimum, which only tightens the bound)
    shared = np.bincount(cl - 1)[cl - 1] > 1
    one_minus_r = np.concatenate([1.0 - np.sum(unit(x[shared]) * unit(cen)[cl[shared] - 1], 1), 1.0 - unit(cen) @ unit(x.mean(0))])
    assert one_minus_r.min() > 0
    tol1 = tol / one_minus_r.min()
    print("CH 1-corr", got1, "oracle", ref1, "relative", abs(got1 - ref1) / ref1, "bound", tol1, "smallest 1 - r", one_minus_r.min())
    assert abs(got1 - ref1) <= tol1 * ref1


def test_calinski_harabasz_of_identical_rows_is_inf(sa):
    x = np.repeat(np.array([[0.0, 1.0, 2.0], [5.0, 5.0, 1.0], [-2.0, 0.5, 9.0]]), [4, 3, 5], axis=0)
    lab = np.repeat([7, 2, 9], [4, 3, 5])
    assert sa.calinski_harabasz(x, lab) == np.inf


def test_dotc_twins(sa):
    """the .C() convention (tests/test_dotc_gpu.py): every argument a pointer, the status last; equal to the plain entries' output"""
    from scipy.spatial.distance import pdist

    L = sa.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)                                     # noqa: E731
    I = lambda *v: np.array(v, np.int32)                                           # noqa: E731
    n, p = 300, 9
    x, labels = gaussian_clusters(3, n, p, 4)
    cl, levels = recode(labels)
    cl = np.ascontiguousarray(cl, np.int32)
    k = levels.size
    for f in ("sharp_C_silhouette_dist", "sharp_C_silhouette", "sharp_C_calinski_harabasz"):
        getattr(L, f).restype = None
    ref = sa.silhouette(labels, data=x, distance="manhattan")
    nb, w, st = np.zeros(n, np.int32), np.zeros(n), I(-1)
    L.sharp_C_silhouette(P(x), P(np.array([float(n)])), P(I(p)), P(I(3)), P(np.array([2.0])), P(cl), P(I(k)), P(nb), P(w), P(st))
    assert st[0] == 0 and np.array_equal(w, ref["sil_width"]) and np.array_equal(levels[nb - 1], ref["neighbor"])
    d = pdist(x, "cityblock")
    refd = sa.silhouette(labels, d=d)
    nb[:], w[:], st[0] = 0, 0, -1
    L.sharp_C_silhouette_dist(P(d), P(I(n)), P(cl), P(I(k)), P(nb), P(w), P(st))
    assert st[0] == 0 and np.array_equal(w, refd["sil_width"]) and np.array_equal(levels[nb - 1], refd["neighbor"])
    for kind, name in ((0, "euclidean"), (1, "1-corr")):
        out = np.zeros(1)
        L.sharp_C_calinski_harabasz(P(x), P(np.array([float(n)])), P(I(p)), P(cl), P(I(k)), P(I(kind)), P(out), P(st))
        assert st[0] == 0 and out[0] == sa.calinski_harabasz(x, labels, distance=name)
    L.sharp_C_silhouette(P(x), P(np.array([float(n)])), P(I(p)), P(I(4)), P(np.array([2.0])), P(cl), P(I(k)), P(nb), P(w), P(st))
    assert st[0] != 0                                                              # canberra


def test_end_to_end_hclust_cutree_silhouette_ch(sa):
    """hclust(x) -> cutree(k = 7) -> silhouette -> calinski_harabasz on 2000 x 30, against scipy / sklearn on the same tree's partition"""
    from scipy.cluster import hierarchy as sch
    from scipy.spatial.distance import pdist
    from sklearn.metrics import calinski_harabasz_score, silhouette_samples

    n, p = 2000, 30
    x, _ = gaussian_clusters(31, n, p, 6)
    tree = sa.hclust(x=x, method="average")
    labels = sa.cutree(tree, k=7)
    sc = sch.fcluster(sch.linkage(pdist(x), "average"), 7, "maxclust")
    assert labels.max() == 7 and labels[0] == 1
    assert len(set(zip(labels.tolist(), sc.tolist()))) == 7                        # the same partition as scipy's tree
    res = sa.silhouette(labels, data=x)
    sk = silhouette_samples(x, labels)
    err = np.abs(res["sil_width"] - sk).max()
    print("end to end: max |width - sklearn|", err, "bound", _tol(n, p))
    assert err <= _tol(n, p)
    ch, ref = sa.calinski_harabasz(x, labels), calinski_harabasz_score(x, labels)
    assert abs(ch - ref) <= 4 * n * p * EPS * ref
    m = sa.cutree(tree, k=[2, 7, 40])                                              # a fine cut: many clusters, several singletons
    fine = sa.silhouette(m[:, 2], data=x)
    reff = sildist(cdist_rows(x, "euclidean"), m[:, 2].astype(np.int64), 40)
    assert np.abs(fine["sil_width"] - reff["width"]).max() <= _tol(n, p)
