"""Times the SNN / Jaccard graph behind the k-NN it is built from -- cfg2's and cfg3's views of tools/bench_umap.py: the
synthetic x1 of 50 000 x 400 and of 500 000 x 70, prepared to 50 columns -- at K = 19 (Seurat's k.param = 20) and prune = 1/15, and
writes profiles/snn_bench.json.

    python tools/bench_snn.py [--shapes 50000x400,500000x70] [--k-param 20] [--prune 0.0666666]

Per shape, in one job and one run per figure (after a warm-up on 2 000 rows): the exact k-NN (tsne_knn, the library's event timer); the
whole snn_graph call on a host clock (two library calls: the count, then count + fill + sort, with the download of the graph) and its
stages from the event timers summed over both calls (snn_reverse and snn_count therefore run twice, snn_fill and snn_sort once); nnz, the
sum of the row work t and the candidate increments per second over the count and the fill passes; the share of rows per row class;
umap_graph + umap_sym on the same lists; louvain_snn and louvain_neighbors on a host clock with their levels, rounds and Q, each one's
ARI against the generating clusters and their ARI against each other.
  build_over_knn    (snn_reverse + snn_count + snn_fill + snn_sort of ONE build: half the first two) / the exact k-NN"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_louvain import profiled  # noqa: E402
from bench_tsne import synth_x1  # noqa: E402

SNN = ("snn_reverse", "snn_count", "snn_fill", "snn_sort")
LV = ("louvain_quantise", "louvain_move", "louvain_state", "louvain_aggregate")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="50000x400,500000x70")
    ap.add_argument("--k-param", type=int, default=20)
    ap.add_argument("--prune", type=float, default=1.0 / 15.0)
    ap.add_argument("--ncl", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snn_bench.json"))
    a = ap.parse_args()
    import sharp_amd
    from sharp_amd.tsne import _knn, _prepare

    um = importlib.import_module("sharp_amd.umap")
    snn = importlib.import_module("sharp_amd.snn")
    sharp_amd.init(0)
    L = sharp_amd.lib()
    K = a.k_param - 1
    wave_cap, block_cap = snn._row_caps()
    rows = []
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        X = synth_x1(n, d, a.ncl, a.seed)
        truth = np.argmax(X[:, :a.ncl], axis=1)
        X = np.ascontiguousarray(_prepare(X, pca=d > 50))                            # (bench_umap.py's preparation of a view)
        sharp_amd.louvain(X[: min(n, 2000)], n_neighbors=a.k_param, graph="snn")      # first call: code objects, allocations
        sharp_amd.louvain(X[: min(n, 2000)], n_neighbors=a.k_param)
        (idx, d2), _, knn = profiled(L, lambda: _knn(X, K), ("tsne_knn",))
        g, wall, st = profiled(L, lambda: sharp_amd.snn_graph(idx, a.prune), SNN)
        deg = 1 + np.bincount(idx.ravel(), minlength=n)
        t = deg + deg[idx].sum(1)
        sum_t = int(t.sum())
        build = st["snn_reverse"]["ms"] / 2 + st["snn_count"]["ms"] / 2 + st["snn_fill"]["ms"] + st["snn_sort"]["ms"]
        passes_ms = st["snn_count"]["ms"] / 2 + st["snn_fill"]["ms"]
        _, _, fz = profiled(L, lambda: um._graph(idx, d2, squared=True), ("umap_graph", "umap_sym"))
        ls, ls_wall, ls_st = profiled(L, lambda: sharp_amd.louvain_snn(idx, a.prune), SNN + LV)
        lf, lf_wall, lf_st = profiled(L, lambda: sharp_amd.louvain_neighbors(idx, d2, squared=True), ("umap_graph", "umap_sym") + LV)
        ari = lambda x, y: round(float(sharp_amd.ARI(x, y)["HA"]), 4)     # noqa: E731
        run = lambda r, w, s: {"call_ms": round(w, 2), "stages": s, "levels": r["levels"],                       # noqa: E731
                               "rounds": sum(l["rounds"] for l in r["levels"]), "n_communities": r["n_communities"],
                               "modularity": r["modularity"], "ari_vs_generating_clusters": ari(truth + 1, r["membership"])}
        row = {"rows": n, "features": d, "features_prepared": int(X.shape[1]), "k_param": a.k_param, "prune": a.prune,
               "knn_ms": knn["tsne_knn"]["ms"], "snn_graph_call_ms": round(wall, 2), "stages_of_both_calls": st,
               "one_build_ms": round(build, 3), "build_over_knn": round(build / knn["tsne_knn"]["ms"], 4),
               "count_twice_costs_ms": round(st["snn_reverse"]["ms"] / 2 + st["snn_count"]["ms"] / 2, 3),
               "nnz": g["nnz"], "sum_t": sum_t, "t_median": int(np.median(t)), "t_max": int(t.max()),
               "increments_per_s_count_and_fill": round(2.0 * (sum_t - n * a.k_param) / (passes_ms * 1e-3), 1),
               "row_class_share": {"wave": round(float((t <= wave_cap).mean()), 6),
                                   "workgroup": round(float(((t > wave_cap) & (t <= block_cap)).mean()), 6),
                                   "dense": round(float((t > block_cap).mean()), 6)},
               "fuzzy_graph": fz, "louvain_snn": run(ls, ls_wall, ls_st), "louvain_neighbors": run(lf, lf_wall, lf_st),
               "ari_snn_vs_fuzzy": ari(ls["membership"], lf["membership"]), "runs_per_figure": 1}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
