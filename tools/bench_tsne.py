"""Per-stage timing of sharp_tsne (the Rtsne behind visualization_SHARP) on synthetic x1 matrices of the clustering configurations'
forview outputs.  One JSON line per size on stdout.

    python tools/bench_tsne.py --n 50000 --d 400 --iters 200      # cfg2's x1: ncl + p ~ 400 columns, through PCA to 50
    python tools/bench_tsne.py --n 500000 --d 70 --iters 30       # cfg3's x1: ncl + 50 columns
    python tools/bench_tsne.py --n 500000 --d 70 --iters 200 --repulsion barnes_hut --theta 0.5
    python tools/bench_tsne.py --n 500000 --d 70 --iters 1000 --repulsion barnes_hut --neighbors    # Rtsne, knn, Rtsne_neighbors once each
    python tools/bench_tsne.py --n 16384 --d 50 --is-distance         # Rtsne's way in from a dist vector: upload, expand, row selection

--neighbors times, on a synchronised host clock and in one process, one Rtsne call, one knn (preparation + exact k-NN, the part that
does not depend on the seed or the optimiser) and one Rtsne_neighbors call on its lists, and says whether the two maps agree bit
for bit.  --is-distance builds the manhattan dist vector of the synthetic rows and reports the stages of knn(d, K, is_distance=True)
from the library's timers, with the row-selection kernel's rate against the n x n matrix it reads.

With --repulsion barnes_hut the repulsion is reported as two stages, the tree build (bh_tree_ms_per_iter) and the traversal
(bh_walk_ms_per_iter); rep_ms_per_iter is their sum.

Stages come from the library's per-kernel HIP-event timers (sharp_profile_*); total_ms is a second, unprofiled call timed on a
synchronised host clock.  Per-iteration figures are the timer totals over the calls they cover; total_1000_est_ms extrapolates the
unprofiled call to max_iter = 1000 from its measured parts (marked as an estimate)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_x1(n, d, ncl, seed):
    """cbind(w * scale(x0), scale(viE))-like: ncl one-hot cluster columns (weighted) + d - ncl noisy projections of cluster centres"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, ncl, n)
    p = d - ncl
    centres = rng.normal(0, 1, size=(ncl, p))
    viE = centres[lab] + 0.5 * rng.normal(size=(n, p))
    x0 = np.zeros((n, ncl))
    x0[np.arange(n), lab] = 1.0
    return np.hstack([2 * (x0 - x0.mean(0)) / x0.std(0, ddof=1), (viE - viE.mean(0)) / viE.std(0, ddof=1)])


def stat(L, name):
    ms, k = C.c_double(), C.c_longlong()
    L.sharp_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return ms.value, k.value


def wall(L, fn):
    L.sharp_synchronize()
    t0 = time.perf_counter()
    r = fn()
    L.sharp_synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def bench_neighbors(sharp_amd, L, X, a):
    from sharp_amd import tsne

    pca = a.d > 50
    loop = dict(perplexity=30, max_iter=a.iters, theta=a.theta, repulsion=a.repulsion)
    sharp_amd.Rtsne(X[: min(a.n, 2000)], **dict(loop, max_iter=2, check_duplicates=False, pca=pca))   # code objects, allocations
    direct, t_direct = wall(L, lambda: sharp_amd.Rtsne(X, check_duplicates=False, pca=pca, **loop))
    (idx, d2), t_knn = wall(L, lambda: tsne._knn(tsne._prepare(X, pca=pca), 90))
    again, t_nn = wall(L, lambda: sharp_amd.Rtsne_neighbors(idx, d2, squared=True, **loop))
    print(json.dumps({"mode": "neighbors", "n": a.n, "d": a.d, "K": 90, "perplexity": 30, "iters": a.iters, "repulsion": a.repulsion,
                      "theta": a.theta, "rtsne_ms": round(t_direct, 1), "knn_with_prepare_ms": round(t_knn, 1),
                      "rtsne_neighbors_ms": round(t_nn, 1), "same_bits": bool(np.array_equal(direct["Y"], again["Y"]))}), flush=True)


def bench_is_distance(sharp_amd, L, X, a):
    n, K = a.n, 90
    d, t_dist = wall(L, lambda: sharp_amd.dist(X, "manhattan"))
    sharp_amd.knn(sharp_amd.dist(X[:2000], "manhattan"), K, is_distance=True)                    # code objects
    L.sharp_profile_enable(1)
    L.sharp_profile_reset()
    _, t_knn = wall(L, lambda: sharp_amd.knn(d, K, is_distance=True, squared=True))
    st = {k: stat(L, k)[0] for k in ["tsne_dist_upload", "dist_expand", "tsne_knn_dist"]}
    L.sharp_profile_enable(0)
    out = {"mode": "is_distance", "n": n, "K": K, "perplexity": 30, "dist_vector_GB": round(n * (n - 1) / 2 * 8 / 1e9, 3),
           "matrix_GB": round(float(n) * n * 8 / 1e9, 3), "make_dist_ms": round(t_dist, 1), "upload_ms": round(st["tsne_dist_upload"], 3),
           "expand_ms": round(st["dist_expand"], 3), "select_ms": round(st["tsne_knn_dist"], 3),
           "select_GB_per_s": round(float(n) * n * 8 / 1e9 / (st["tsne_knn_dist"] * 1e-3), 1), "knn_call_wall_ms": round(t_knn, 1)}
    if a.iters > 0:
        _, t_map = wall(L, lambda: sharp_amd.Rtsne(d, is_distance=True, perplexity=30, max_iter=a.iters, theta=a.theta, repulsion=a.repulsion))
        out.update({"iters": a.iters, "repulsion": a.repulsion, "rtsne_is_distance_ms": round(t_map, 1)})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--d", type=int, default=400)
    ap.add_argument("--ncl", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repulsion", choices=["exact", "barnes_hut"], default="exact")
    ap.add_argument("--theta", type=float, default=0.5)
    ap.add_argument("--neighbors", action="store_true", help="time Rtsne, knn and Rtsne_neighbors once each")
    ap.add_argument("--is-distance", action="store_true", help="time the stages of the k-NN from a dist vector")
    a = ap.parse_args()
    import sharp_amd

    sharp_amd.init(0)
    L = sharp_amd.lib()
    X = synth_x1(a.n, a.d, a.ncl, a.seed)
    if a.neighbors:
        return bench_neighbors(sharp_amd, L, X, a)
    if a.is_distance:
        return bench_is_distance(sharp_amd, L, X, a)
    kw = dict(perplexity=30, max_iter=a.iters, check_duplicates=False, pca=a.d > 50, theta=a.theta, repulsion=a.repulsion)
    sharp_amd.Rtsne(X[: min(a.n, 2000)], **dict(kw, max_iter=2))       # first call: code objects, allocations
    L.sharp_profile_enable(1)
    L.sharp_profile_reset()
    sharp_amd.Rtsne(X, **kw)
    L.sharp_synchronize()
    st = {k: stat(L, k) for k in ["tsne_pca", "tsne_normalize", "tsne_knn", "tsne_calib", "tsne_sym", "tsne_attr", "tsne_rep", "tsne_update",
                                  "tsne_kl", "tsne_bh_tree", "tsne_bh_walk"]}
    eig = stat(L, "host:tsne_pca_eigen")
    L.sharp_profile_enable(0)
    t0 = time.perf_counter()
    sharp_amd.Rtsne(X, **kw)
    total = (time.perf_counter() - t0) * 1e3
    per = lambda k: st[k][0] / max(st[k][1], 1)                       # noqa: E731
    rep_ms = per("tsne_bh_tree") + per("tsne_bh_walk") if a.repulsion == "barnes_hut" else per("tsne_rep")
    iter_ms = per("tsne_attr") + rep_ms + per("tsne_update")
    fixed = st["tsne_pca"][0] + st["tsne_normalize"][0] + st["tsne_knn"][0] + st["tsne_calib"][0] + st["tsne_sym"][0]
    loop = total - fixed
    out = {"n": a.n, "d": a.d, "dims": 2, "perplexity": 30, "iters": a.iters, "repulsion": a.repulsion, "theta": a.theta,
           "pca_ms": round(st["tsne_pca"][0], 3), "pca_eigen_host_ms": round(eig[0], 3), "normalize_ms": round(st["tsne_normalize"][0], 3),
           "knn_ms": round(st["tsne_knn"][0], 3), "calib_ms": round(st["tsne_calib"][0], 3), "sym_ms": round(st["tsne_sym"][0], 3),
           "attr_ms_per_iter": round(per("tsne_attr"), 4), "rep_ms_per_iter": round(rep_ms, 4),
           "bh_tree_ms_per_iter": round(per("tsne_bh_tree"), 4), "bh_walk_ms_per_iter": round(per("tsne_bh_walk"), 4),
           "update_ms_per_iter": round(per("tsne_update"), 4), "kl_ms_per_eval": round(per("tsne_kl"), 4),
           "iter_ms": round(iter_ms, 4), "rep_pairs_per_s": float(f"{a.n * a.n / (rep_ms * 1e-3):.4g}"),
           "knn_pairs_per_s": float(f"{a.n * a.n / (st['tsne_knn'][0] * 1e-3):.4g}"),
           "total_ms": round(total, 2), "loop_ms_per_iter_unprofiled": round(loop / max(a.iters, 1), 4),
           "total_1000_est_ms": round(fixed + 1000 * loop / max(a.iters, 1), 1), "total_1000_is_estimate": a.iters != 1000}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
