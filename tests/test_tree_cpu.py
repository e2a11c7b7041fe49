"""CPU tests of the tree / plot_markers feature: the HCASS2 restatement on the oracle's agglomeration, the selection part
of plot_markers (runs without a device), get_percluster_exp and the R side's definitions."""
import os
import re

import numpy as np
import pytest

from _tree_ref import cut, hcass2, leaves, percluster, plot_markers_select, same_partition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ["ward.D", "single", "complete", "average", "mcquitty", "median", "centroid", "ward.D2"]


@pytest.mark.parametrize("method", METHODS)
def test_hcass2_on_oracle_hclust(oracle, method):
    from scipy.cluster import hierarchy as sch
    from scipy.spatial.distance import pdist

    n = 300
    x = np.random.default_rng(4).normal(size=(n, 6))
    x[:40] += 3.0
    d = pdist(x)
    ia, ib, crit = oracle.hclust(d, n, method)
    merge, order = hcass2(ia, ib)
    assert np.array_equal(np.sort(order), np.arange(1, n + 1))
    pos = np.empty(n + 1, np.int64)
    pos[order] = np.arange(n)
    lv = leaves(merge)
    for i, (a, b) in enumerate(merge):
        la = np.array([-a]) if a < 0 else lv[a - 1]
        lb = np.array([-b]) if b < 0 else lv[b - 1]
        pa, pb = np.sort(pos[la]), np.sort(pos[lb])
        assert np.array_equal(pa, np.arange(pa[0], pa[0] + pa.size)) and np.array_equal(pb, np.arange(pb[0], pb[0] + pb.size))
        assert pa[-1] + 1 == pb[0]                            # the first member immediately left of the second
        assert not (a > 0 and b < 0)                          # a singleton before a cluster
        if (a < 0) == (b < 0):
            assert abs(a) < abs(b)                            # two singletons, two clusters: ascending
        assert (a < 0 or a <= i) and (b < 0 or b <= i)        # only earlier steps
    if method in ("median", "centroid"):                      # (scipy's centroid / median assume squared Euclidean input: another criterion)
        return
    if method == "ward.D":                                    # scipy's ward on sqrt(d): its squared heights are ward.D's
        Z = sch.linkage(np.sqrt(d), "ward")
        np.testing.assert_allclose(Z[:, 2] ** 2, crit, rtol=1e-12)
    else:
        Z = sch.linkage(d, {"mcquitty": "weighted", "ward.D2": "ward"}.get(method, method))
        np.testing.assert_allclose(Z[:, 2], crit, rtol=1e-12)
    for k in range(2, 11):
        assert same_partition(cut(merge, k), sch.fcluster(Z, k, "maxclust")), k


def _sginfo(seed=0, ncell=90, logmark=True):
    rng = np.random.default_rng(seed)
    label = rng.integers(1, 5, ncell)
    label[:4] = [1, 2, 3, 4]
    ng = 17
    mg = {"gene": np.array(["g%d" % i for i in range(ng)]), "icluster": np.array([1] * 6 + [2] * 2 + [3] * 5 + [4] * 4),
          "auc": np.round(rng.random(ng), 1),                # ties in auc
          "pvalue": rng.random(ng) * 1e-3}
    mat = rng.poisson(3.0, size=(ng, ncell)).astype(np.float64)
    mat[9] = 3.0                                              # a zero-sd row (cluster 3); 3 and log2(3 + 1) sum exactly
    return {"mginfo": mg, "mat": mat, "label": label, "logmark": logmark}


def _same(res, ref, sg):
    for k, v in sg["mginfo"].items():
        assert np.array_equal(res["sortmarker"][k], np.asarray(v)[ref["sortmarker_rows"]]), k
    assert res["genes"].tolist() == ref["genes"] and res["cells"].tolist() == ref["cells"]
    np.testing.assert_allclose(res["sm"], ref["sm"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("logmark", [True, False])
def test_plot_markers_selection_matches_restatement(logmark):
    from sharp_amd.tree import _plot_markers_select

    sg = _sginfo(logmark=logmark)
    assert np.unique(sg["mginfo"]["auc"]).size < 17
    for kw in ({}, {"N_marker": 4}, {"N_marker": 3, "sN_cluster": 2}, {"sN_cluster": 3}):
        res = _plot_markers_select(sg, **kw)
        ref = plot_markers_select(sg, **kw)
        _same(res, ref, sg)
        assert "g9" not in res["genes"].tolist()              # the zero-sd row is dropped
    res = _plot_markers_select(sg, N_marker=4)
    assert np.count_nonzero(res["sortmarker"]["icluster"] == 2) == 2 and res["sm"].shape[0] == 4 + 2 + 3 + 4   # a cluster with fewer markers
    # the argument wins over sginfo["logmark"]
    _same(_plot_markers_select(sg, logmark=not logmark), plot_markers_select(sg, logmark=not logmark), sg)


def test_plot_markers_sampling_above_10000_cells_and_refusals():
    import sharp_amd
    from sharp_amd.tree import _plot_markers_select

    sg = _sginfo(seed=3, ncell=10007)
    res = _plot_markers_select(sg, sN_cluster=3)
    ref = plot_markers_select(sg, sN_cluster=3)
    _same(res, ref, sg)
    cnt = [np.count_nonzero(sg["label"] == c) for c in (1, 2, 3)]
    assert res["cells"].size == sum(int(np.ceil(c * 1e4 / 10007)) for c in cnt) and res["ncells"] == 10007
    _same(_plot_markers_select(sg, nratio=0.013), plot_markers_select(sg, nratio=0.013), sg)
    for bad in (0, -0.5, 1.5, float("nan")):
        with pytest.raises(sharp_amd.SharpError, match="nratio"):
            _plot_markers_select(sg, nratio=bad)
    sg["logmark"] = None
    with pytest.raises(sharp_amd.SharpError, match="logmark"):
        _plot_markers_select(sg)


def test_plot_markers_needs_a_device():
    import torch

    import sharp_amd

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(sharp_amd.SharpError):
        sharp_amd.plot_markers(_sginfo(), plot=False)
    with pytest.raises(sharp_amd.SharpError):
        sharp_amd.dist(np.zeros((3, 2)))
    with pytest.raises(sharp_amd.SharpError):
        sharp_amd.hclust(x=np.eye(3))


def test_get_percluster_exp():
    import scipy.sparse as sp

    import sharp_amd

    rng = np.random.default_rng(1)
    blocks = [rng.poisson(1.0, size=(7, k)).astype(np.float64) for k in (5, 8, 3)]
    lab = np.array([2, 2, 5, 9, 2] + [5, 5, 2, 2, 9, 9, 5, 2] + [2, 5, 5])          # cluster 9 is missing from the last block
    ref = percluster(blocks, lab)
    got = sharp_amd.get_percluster_exp(blocks, {"pred_clusters": lab})
    assert len(got) == 3 and all(np.array_equal(g, r) for g, r in zip(got, ref))
    gs = sharp_amd.get_percluster_exp([sp.csc_matrix(b) for b in blocks], lab)
    assert all(sp.issparse(g) and np.array_equal(g.toarray(), r) for g, r in zip(gs, ref))
    gm = sharp_amd.get_percluster_exp([blocks[0], sp.csr_matrix(blocks[1]), blocks[2]], lab)
    assert all(np.array_equal(np.asarray(g), r) for g, r in zip(gm, ref))
    lab2 = np.concatenate([lab, [11]])                        # a cluster held by no block
    g2 = sharp_amd.get_percluster_exp(blocks, lab2)
    assert len(g2) == 4 and g2[3] is None and all(np.array_equal(g, r) for g, r in zip(g2[:3], ref))


def test_r_side_defines_the_new_functions():
    src = open(os.path.join(ROOT, "r", "sharp_hip.R")).read()
    for name in ("sharp_dist", "sharp_hclust", "sharp_plot_markers"):
        assert re.search(r"^%s <- function\(" % name, src, re.M), name
    formals = re.search(r"^sharp_plot_markers <- function\(([^)]*)\)", src, re.M).group(1)
    names = [a.split("=")[0].strip() for a in formals.split(",")]
    assert names == ["sginfo", "label", "N.marker", "sN.cluster", "filename", "filetype", "nratio", "n.cores", "width", "height", "..."]
    assert 'class = "hclust"' in src and "sharp_C_hclust" in src and "sharp_C_dist" in src
