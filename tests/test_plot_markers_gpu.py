"""plot_markers end to end on the GPU (R/plot_markers.R:38-242): selection against the literal restatement, both trees against HCASS2 of
the oracle's agglomeration run on the GPU's own dist output, and the figure file."""
import os

import numpy as np
import pytest

from _tree_ref import hcass2, plot_markers_select

pytestmark = pytest.mark.gpu
SEED = 20261003


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


def _blank(path, filetype, width, height):
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure

    fig = Figure(figsize=(7, 7) if filetype == "pdf" else (width / 100.0, height / 100.0), dpi=100)
    FigureCanvasAgg(fig)
    fig.savefig(path, format=filetype)
    return os.path.getsize(path)


@pytest.mark.parametrize("n,filetype", [(3000, "pdf"), (12000, "png")])
def test_plot_markers_end_to_end(sa, oracle, tmp_path, n, filetype):
    m, G = 600, 5
    X = oracle.synth_fill(SEED, m, 0, n, G, 150) + np.random.default_rng(n).uniform(0, 1e-3, size=(m, n))
    truth = oracle.synth_cluster(SEED, range(n), G) + 1
    sg = sa.get_marker_genes(X, {"pred_clusters": truth}, gene_names=["g%d" % i for i in range(m)])
    assert np.unique(sg["mginfo"]["icluster"]).size >= 2
    f = str(tmp_path / f"heat.{filetype}")
    res = sa.plot_markers(sg, filename=f, logmark=True)
    ref = plot_markers_select(sg, logmark=True)
    for k, v in sg["mginfo"].items():
        assert np.array_equal(res["sortmarker"][k], np.asarray(v)[ref["sortmarker_rows"]]), k
    assert res["genes"].tolist() == ref["genes"] and res["cells"].tolist() == ref["cells"]
    np.testing.assert_allclose(res["sm"], ref["sm"], rtol=0, atol=1e-12)
    if n > 10000:
        assert res["cells"].size < n and res["cells"].size <= 10000 + G
    for tree, obs in ((res["row_tree"], res["sm"]), (res["col_tree"], np.ascontiguousarray(res["sm"].T))):
        d = sa.dist(obs)                                     # the GPU's own distances: the agglomeration is compared on identical bits
        ia, ib, crit = oracle.hclust(d, obs.shape[0], "ward.D")
        merge, order = hcass2(ia, ib)
        assert np.array_equal(tree["merge"], merge) and np.array_equal(tree["order"], order)
        np.testing.assert_allclose(tree["height"], crit, rtol=1e-9, atol=1e-12)
    assert res["filename"] == f and open(f, "rb").read(4) == (b"%PDF" if filetype == "pdf" else b"\x89PNG")
    assert os.path.getsize(f) > _blank(str(tmp_path / f"blank.{filetype}"), filetype, 900, 900)
    again = sa.plot_markers(sg, logmark=True, plot=False)
    assert again["filename"] is None
    for t in ("row_tree", "col_tree"):
        for key in ("merge", "order", "height"):
            assert np.array_equal(again[t][key], res[t][key])


def test_plot_markers_default_file_and_too_many_cells(sa, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(2)
    n = 400
    lab = np.repeat([1, 2], n // 2)
    mat = rng.gamma(2.0, 1.0, size=(12, n)) + (lab == 1) * np.arange(12)[:, None]
    sg = {"mginfo": {"gene": np.array(["g%d" % i for i in range(12)]), "auc": rng.random(12), "icluster": np.repeat([1, 2], 6),
                     "pvalue": rng.random(12) * 1e-3}, "mat": mat, "label": lab, "logmark": False}
    res = sa.plot_markers(sg)
    assert res["filename"] == "markers_heatmap.pdf" and os.path.exists("markers_heatmap.pdf")
    big = dict(sg, mat=np.zeros((12, 17000)), label=np.repeat([1, 2], 8500))
    big["mat"] = rng.random((12, 17000))
    with pytest.raises(sa.SharpError, match="nratio"):
        sa.plot_markers(big, nratio=1.0, plot=False)
