"""Times louvain_neighbors on the neighbour graphs the maps are built from -- cfg2's and cfg3's views of
tools/bench_umap.py: the synthetic x1 of 50 000 x 400 and of 500 000 x 70, prepared as visualization_SHARP prepares them (Rtsne's
preparation: PCA to 50 columns, normalisation), n_neighbors = 15 -- and writes profiles/louvain_bench.json.

    python tools/bench_louvain.py [--shapes 50000x400,500000x70] [--n-neighbors 15] [--reps 2]

Per shape, in one job: the exact k-NN (tsne_knn, the library's event timer), the whole louvain_neighbors call on a host clock (the
faster of --reps calls after a warm-up on 2 000 rows; it starts from host lists and ends in a download), its stages from the event
timers of the faster call (umap_graph + umap_sym: the fuzzy graph; louvain_quantise; louvain_move: the local-moving kernels of all
rounds; louvain_state: totals, internal weights, the sort of the terms, Q and the host's read of it, all rounds; louvain_aggregate),
the levels with their rounds, and one umap_epochs epoch (epoch 100 of 200) on the same graph.  The two ratios the issue asks for:
  move_round_over_epoch      louvain_move per round / one UMAP epoch
  round_over_epoch           (louvain_move + louvain_state) per round / one UMAP epoch
  louvain_over_knn           the whole call / the exact k-NN"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_tsne import stat, synth_x1  # noqa: E402

STAGES = ("umap_graph", "umap_sym", "louvain_quantise", "louvain_move", "louvain_state", "louvain_aggregate")


def profiled(L, fn, names):
    L.sharp_profile_enable(1)
    L.sharp_profile_reset()
    L.sharp_synchronize()
    t0 = time.perf_counter()
    out = fn()
    wall = (time.perf_counter() - t0) * 1e3
    L.sharp_synchronize()
    got = {k: {"ms": round(stat(L, k)[0], 3), "launches": int(stat(L, k)[1])} for k in names}
    L.sharp_profile_enable(0)
    return out, wall, got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="50000x400,500000x70")
    ap.add_argument("--n-neighbors", type=int, default=15)
    ap.add_argument("--ncl", type=int, default=20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "louvain_bench.json"))
    a = ap.parse_args()
    import sharp_amd
    from sharp_amd.tsne import _knn, _prepare

    um = importlib.import_module("sharp_amd.umap")
    sharp_amd.init(0)
    L = sharp_amd.lib()
    K = a.n_neighbors - 1
    rows = []
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        X = synth_x1(n, d, a.ncl, a.seed)
        truth = np.argmax(X[:, :a.ncl], axis=1)
        X = np.ascontiguousarray(_prepare(X, pca=d > 50))                            # (bench_umap.py's preparation of a view)
        sharp_amd.louvain(X[: min(n, 2000)], n_neighbors=a.n_neighbors)               # first call: code objects, allocations
        (idx, d2), _, knn = profiled(L, lambda: _knn(X, K), ("tsne_knn",))
        best = None
        for _ in range(a.reps):
            out, wall, st = profiled(L, lambda: sharp_amd.louvain_neighbors(idx, d2, squared=True), STAGES)
            if best is None or wall < best[1]:
                best = (out, wall, st)
        out, wall, st = best
        rounds = sum(l["rounds"] for l in out["levels"])
        rp, col, val = um._graph(idx, d2, squared=True)[:3]
        ab = sharp_amd.umap_ab()
        Y0 = np.random.default_rng(a.seed).uniform(0.0, 10.0, size=(n, 2))
        um._epochs(rp, col, val, Y0, 200, 100, 101, *ab)
        _, _, ep = profiled(L, lambda: um._epochs(rp, col, val, Y0, 200, 100, 101, *ab), ("umap_epochs",))
        epoch_ms = ep["umap_epochs"]["ms"]
        move_round = st["louvain_move"]["ms"] / max(rounds, 1)
        full_round = (st["louvain_move"]["ms"] + st["louvain_state"]["ms"]) / max(rounds, 1)
        row = {"rows": n, "features": d, "features_prepared": int(X.shape[1]), "n_neighbors": a.n_neighbors, "nnz": int(col.size),
               "knn_ms": knn["tsne_knn"]["ms"],
               "louvain_call_ms": round(wall, 2), "stages": st, "levels": out["levels"], "rounds": rounds,
               "n_communities": out["n_communities"], "modularity": out["modularity"],
               "ari_vs_generating_clusters": round(float(sharp_amd.ARI(truth + 1, out["membership"])["HA"]), 4),
               "move_round_ms": round(move_round, 4), "round_ms": round(full_round, 4), "umap_epoch_ms": epoch_ms,
               "move_round_over_epoch": round(move_round / epoch_ms, 3), "round_over_epoch": round(full_round / epoch_ms, 3),
               "louvain_over_knn": round(wall / knn["tsne_knn"]["ms"], 4), "reps": a.reps}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
