"""Per-stage timing of sharp_umap (uwot::umap beside Rtsne) on synthetic x1 matrices of the clustering configurations'
forview outputs, as tools/bench_tsne.py does for Rtsne.  One JSON line per size on stdout.

    python tools/bench_umap.py --n 50000 --d 400        # cfg2's view: ncl + p ~ 400 columns, through PCA to 50
    python tools/bench_umap.py --n 500000 --d 70        # cfg3's view: ncl + 50 columns
    python tools/bench_umap.py --n 50000 --d 400 --neighbors   # umap, knn and umap_neighbors once each, and whether the maps agree

The input is prepared as visualization_SHARP(method="umap") prepares it (Rtsne's preparation: PCA to 50 when d > 50, normalisation).
Stages come from the library's per-kernel HIP-event timers (sharp_profile_*): the k-NN is Rtsne's own stage (tsne_knn), umap_graph
(rho, sigma, weights), umap_sym (sort, union, CSR), umap_sqrt (the lists' distances from their squares) and umap_epochs are UMAP's; host:umap_init is the start (download, PCA, scaling).
total_ms is a second, unprofiled call timed on a synchronised host clock.  pair_terms_per_s counts the (edge, term) slots the epoch
kernel visits, nnz * (1 + negative_sample_rate) per epoch, fired or not.  Host work between the stages (uploads,
downloads, the PCA's eigensolver) is in total_ms only, so the stages do not add up to it."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_tsne import stat, synth_x1, wall  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--d", type=int, default=400)
    ap.add_argument("--ncl", type=int, default=20)
    ap.add_argument("--n-neighbors", type=int, default=15)
    ap.add_argument("--negative-sample-rate", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=None, help="default: uwot's rule (500 up to 10 000 rows, else 200)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--neighbors", action="store_true", help="time umap, knn and umap_neighbors once each")
    a = ap.parse_args()
    import sharp_amd
    from sharp_amd.tsne import _knn, _prepare

    sharp_amd.init(0)
    L = sharp_amd.lib()
    X = synth_x1(a.n, a.d, a.ncl, a.seed)
    K = a.n_neighbors - 1
    kw = dict(n_neighbors=a.n_neighbors, n_epochs=a.epochs, negative_sample_rate=a.negative_sample_rate)
    sharp_amd.umap(X[: min(a.n, 2000)], **dict(kw, n_epochs=2))        # first call: code objects, allocations
    Xp, t_prep = wall(L, lambda: _prepare(X, pca=a.d > 50))
    if a.neighbors:
        Y0 = np.random.default_rng(a.seed).normal(size=(a.n, 2))
        direct, t_direct = wall(L, lambda: sharp_amd.umap(Xp, init=Y0, **kw))
        (idx, d2), t_knn = wall(L, lambda: _knn(Xp, K))
        again, t_nn = wall(L, lambda: sharp_amd.umap_neighbors(idx, d2, squared=True, init=Y0, n_epochs=a.epochs,
                                                               negative_sample_rate=a.negative_sample_rate))
        print(json.dumps({"mode": "neighbors", "n": a.n, "d": a.d, "n_neighbors": a.n_neighbors, "n_epochs": direct["n_epochs"],
                          "prepare_ms": round(t_prep, 1), "umap_ms": round(t_direct, 1), "knn_ms": round(t_knn, 1),
                          "umap_neighbors_ms": round(t_nn, 1), "same_bits": bool(np.array_equal(direct["Y"], again["Y"]))}), flush=True)
        return
    L.sharp_profile_enable(1)
    L.sharp_profile_reset()
    out = sharp_amd.umap(Xp, ret_nn=True, **kw)
    L.sharp_synchronize()
    st = {k: stat(L, k) for k in ["tsne_knn", "umap_sqrt", "umap_graph", "umap_sym", "umap_epochs", "host:umap_init", "host:umap_ab", "tsne_pca"]}
    L.sharp_profile_enable(0)
    # the entries of A + A^T: 2 n K less one for every pair that names each other
    rows = np.repeat(np.arange(a.n, dtype=np.int64), K)
    cols = out["nn"]["index"].reshape(-1).astype(np.int64)
    nnz = int(np.unique(np.concatenate([rows * a.n + cols, cols * a.n + rows])).size)
    T = 1 + a.negative_sample_rate
    _, total = wall(L, lambda: sharp_amd.umap(Xp, **kw))
    ep = out["n_epochs"]
    ep_ms = st["umap_epochs"][0] / max(ep, 1)
    print(json.dumps({"n": a.n, "d": a.d, "d_prepared": int(Xp.shape[1]), "dims": 2, "n_neighbors": a.n_neighbors, "n_epochs": ep,
                      "negative_sample_rate": a.negative_sample_rate, "nnz": nnz, "prepare_wall_ms": round(t_prep, 1), "knn_ms": round(st["tsne_knn"][0], 3),
                      "knn_pairs_per_s": float(f"{a.n * a.n / (st['tsne_knn'][0] * 1e-3):.4g}"),
                      "init_host_ms": round(st["host:umap_init"][0], 3), "init_pca_ms": round(st["tsne_pca"][0], 3),
                      "ab_host_ms": round(st["host:umap_ab"][0], 3), "sqrt_ms": round(st["umap_sqrt"][0], 3), "graph_ms": round(st["umap_graph"][0], 3),
                      "sym_ms": round(st["umap_sym"][0], 3), "epochs_ms": round(st["umap_epochs"][0], 3), "epoch_ms": round(ep_ms, 4),
                      "pair_terms_per_s": float(f"{nnz * T / (ep_ms * 1e-3):.4g}"), "total_ms": round(total, 2)}), flush=True)


if __name__ == "__main__":
    main()
