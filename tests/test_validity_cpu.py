"""CPU tests of cutree / silhouette / calinski_harabasz: cutree needs no device and is checked here against the tree tests'
partition helper and R's numbering rule; the two evaluation functions must refuse to run without a device; the R side's definitions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from _tree_ref import cut, hcass2, same_partition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ["ward.D", "single", "complete", "average", "mcquitty", "median", "centroid", "ward.D2"]


def _tree(oracle, method, n, seed=4):
    from scipy.spatial.distance import pdist

    x = np.random.default_rng(seed).normal(size=(n, 6))
    x[: n // 8] += 3.0
    ia, ib, crit = oracle.hclust(pdist(x), n, method)
    merge, order = hcass2(ia, ib)
    return {"merge": merge, "height": crit, "order": order, "method": method, "n": n}


def _numbered_by_first_appearance(lab):
    """observation 1 is in cluster 1; each new label is the previous maximum + 1"""
    top = 0
    for v in lab.tolist():
        if v > top:
            if v != top + 1:
                return False
            top = v
    return lab[0] == 1


@pytest.mark.parametrize("n", [300, 2000])
@pytest.mark.parametrize("method", METHODS)
def test_cutree_k_matches_the_partition_and_r_numbering(oracle, method, n):
    import sharp_amd

    t = _tree(oracle, method, n)
    ks = [1, 2, 7, n - 1, n]
    for k in ks:
        lab = sharp_amd.cutree(t, k=k)
        assert lab.dtype == np.int32 and lab.shape == (n,)
        assert lab.max() == k and same_partition(lab, cut(t["merge"], k)), k
        assert _numbered_by_first_appearance(lab), k
    m = sharp_amd.cutree(t, k=ks[::-1])                        # a vector of k: one column per value, in the order given
    assert m.shape == (n, len(ks)) and m.dtype == np.int32
    for j, k in enumerate(ks[::-1]):
        assert np.array_equal(m[:, j], sharp_amd.cutree(t, k=k))


@pytest.mark.parametrize("method", ["ward.D", "average", "single", "complete"])
def test_cutree_h_is_k_by_r_formula(oracle, method):
    import sharp_amd

    n = 300
    t = _tree(oracle, method, n)
    ht = t["height"]
    assert np.all(np.diff(ht) >= 0)
    hs = [ht[0] / 2, ht[0], (ht[10] + ht[11]) / 2, ht[11], ht[n - 3], (ht[n - 3] + ht[n - 2]) / 2, ht[n - 2], ht[n - 2] * 2]
    ext = np.append(ht, np.inf)
    for h in hs:
        k = n + 1 - (int(np.flatnonzero(ext > h)[0]) + 1)      # k = n + 1 - which.max(c(height, Inf) > h)
        assert np.array_equal(sharp_amd.cutree(t, h=h), sharp_amd.cutree(t, k=k)), h
    assert sharp_amd.cutree(t, h=hs[0]).max() == n and sharp_amd.cutree(t, h=hs[-1]).max() == 1
    m = sharp_amd.cutree(t, h=hs)
    assert m.shape == (n, len(hs)) and all(np.array_equal(m[:, j], sharp_amd.cutree(t, h=h)) for j, h in enumerate(hs))
    assert np.array_equal(sharp_amd.cutree(t, k=5, h=hs[0]), sharp_amd.cutree(t, k=5))      # k wins


def test_cutree_errors_and_inversions(oracle):
    import sharp_amd

    n = 300
    t = _tree(oracle, "average", n)
    with pytest.raises(sharp_amd.SharpError, match="either 'k' or 'h' must be specified"):
        sharp_amd.cutree(t)
    for bad in (0, n + 1, [2, n + 1]):
        with pytest.raises(sharp_amd.SharpError, match="elements of 'k' must be between 1 and %d" % n):
            sharp_amd.cutree(t, k=bad)
    c = None
    for seed in range(4, 40):                                  # a centroid tree with an inversion
        c = _tree(oracle, "centroid", n, seed)
        if np.any(np.diff(c["height"]) < 0):
            break
    assert np.any(np.diff(c["height"]) < 0)
    with pytest.raises(sharp_amd.SharpError, match=r"the 'height' component of 'tree' is not sorted \(increasingly\)"):
        sharp_amd.cutree(c, h=float(np.median(c["height"])))
    lab = sharp_amd.cutree(c, k=9)
    assert same_partition(lab, cut(c["merge"], 9)) and _numbered_by_first_appearance(lab)


def test_sharp_cutree_c_abi_needs_no_device():
    """the plain C entry, never initialised: sharp_cutree works where sharp_init has not run (or cannot)"""
    import sharp_amd

    L = C.CDLL(sharp_amd.so_path())
    L.sharp_last_error.restype = C.c_char_p
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))        # noqa: E731
    merge = np.asfortranarray(np.array([[-1, -2], [-3, -4], [1, 2], [-5, 3]], np.int32))
    k = np.array([5, 3, 2, 1], np.int32)
    out = np.zeros((4, 5), np.int32)
    assert L.sharp_cutree(ip(merge), 5, ip(k), 4, ip(out)) == 0
    assert out.tolist() == [[1, 2, 3, 4, 5], [1, 1, 2, 2, 3], [1, 1, 1, 1, 2], [1, 1, 1, 1, 1]]
    k[0] = 6
    assert L.sharp_cutree(ip(merge), 5, ip(k), 4, ip(out)) == 2 and b"between 1 and 5" in L.sharp_last_error()
    merge[2, 0] = 4                                            # a step that refers to a later one
    assert L.sharp_cutree(ip(merge), 5, ip(k[1:]), 3, ip(out)) == 2 and b"invalid 'tree'" in L.sharp_last_error()


def test_silhouette_and_ch_need_a_device():
    import torch

    import sharp_amd

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x = np.random.default_rng(0).normal(size=(12, 3))
    lab = np.arange(12) % 3
    with pytest.raises(sharp_amd.SharpError):
        sharp_amd.silhouette(lab, data=x)
    with pytest.raises(sharp_amd.SharpError):
        sharp_amd.silhouette(lab, d=np.ones(66))
    with pytest.raises(sharp_amd.SharpError):
        sharp_amd.calinski_harabasz(x, lab)
    with pytest.raises(sharp_amd.SharpError):
        sharp_amd.calinski_harabasz(x, lab, distance="1-corr")
    # refusals that need no device come first
    with pytest.raises(sharp_amd.SharpError, match="'x' must only have integer codes"):
        sharp_amd.silhouette(lab + 0.5, data=x)
    with pytest.raises(sharp_amd.SharpError, match="data="):
        sharp_amd.silhouette(np.zeros(46341, np.int64), d=np.broadcast_to(np.float64(1.0), (46341 * 46340 // 2,)))
    assert sharp_amd.silhouette(np.ones(12, np.int64), data=x) is None


def test_r_side_defines_the_validity_functions():
    src = open(os.path.join(ROOT, "r", "sharp_hip.R")).read()
    for name in ("sharp_silhouette", "sharp_calinski_harabasz"):
        assert re.search(r"^%s <- function\(" % name, src, re.M), name
    formals = re.search(r"^sharp_silhouette <- function\(([^)]*)\)", src, re.M).group(1)
    names = [a.split("=")[0].strip() for a in formals.split(",")]
    assert names[:3] == ["x", "dist", "data"] and "distance" in names and "p" in names
    formals = re.search(r"^sharp_calinski_harabasz <- function\(([^)]*)\)", src, re.M).group(1)
    assert [a.split("=")[0].strip() for a in formals.split(",")] == ["data", "labels", "distance"]
    for sym in ("sharp_C_silhouette_dist", "sharp_C_silhouette", "sharp_C_calinski_harabasz"):
        assert '"%s"' % sym in src, sym
    assert 'class = "silhouette"' in src
