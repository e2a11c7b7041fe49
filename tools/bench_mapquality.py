"""Times the neighbour-rank pass behind trustworthiness() / continuity() at the sizes the maps are built for -- the
views SHARP returns for cfg2 (50 000 x 50) and cfg3 (500 000 x 50), the synthetic x1 of tools/bench_umap.py at d = 50 -- with K = 15,
and writes profiles/mapquality_bench.json.

    python tools/bench_mapquality.py [--shapes 50000x50,500000x50] [--k 15] [--reps 2]

Per shape, from the library's event timers (sharp_profile_*), each after a warm-up call on 2 000 rows, the minimum of --reps calls:
  ranks_good     neighbor_ranks(X, knn(X, K)): the good-map case, nearly every pair leaves the epilogue at its first compare
  ranks_random   neighbor_ranks(X, seeded random well-formed lists): the worst case, about half the pairs reach the search
  ranks_d2       neighbor_ranks(Y, knn(X, K)), Y the n x 2 map: continuity's pass
  silhouette     sil_tile_kernel (euclidean) on the same X in the same job: the same pair loop with another epilogue, the yardstick
and the whole trustworthiness(X, Y, K) call on a host clock (it ends in a download).  Y is X's first two principal components: a
map of middling quality that costs no UMAP run here.  pairs_per_s = n^2 / the tile kernel's time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_tsne import stat, synth_x1  # noqa: E402

NR = ("nr_threshold_kernel", "nr_tile_kernel", "nr_finish_kernel")


def random_lists(n, K, seed):
    """K distinct rows other than the row itself, drawn for all rows at once; rows with a repeated index are drawn again"""
    rng = np.random.default_rng(seed)
    own = np.arange(n)[:, None]
    c = rng.integers(0, n - 1, size=(n, K))
    while True:
        s = np.sort(c, axis=1)
        again = np.flatnonzero((s[:, 1:] == s[:, :-1]).any(axis=1))
        if again.size == 0:
            return np.ascontiguousarray(c + (c >= own), np.int32)
        c[again] = rng.integers(0, n - 1, size=(again.size, K))


def profiled(L, fn, names, reps):
    """the event-timer totals of `names` over one call of fn: the call with the smallest sum out of reps"""
    best = None
    for _ in range(reps):
        L.sharp_profile_enable(1)
        L.sharp_profile_reset()
        fn()
        L.sharp_synchronize()
        got = {k: round(stat(L, k)[0], 3) for k in names}
        got["launches"] = int(stat(L, names[-2] if len(names) > 1 else names[0])[1])
        L.sharp_profile_enable(0)
        if best is None or sum(got[k] for k in names) < sum(best[k] for k in names):
            best = got
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="50000x50,500000x50")
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--ncl", type=int, default=20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapquality_bench.json"))
    a = ap.parse_args()
    import sharp_amd

    sharp_amd.init(0)
    L = sharp_amd.lib()
    K = a.k
    rows = []
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        X = np.ascontiguousarray(synth_x1(n, d, a.ncl, a.seed))
        lab = np.argmax(X[:, :a.ncl], axis=1) + 1
        Xc = X - X.mean(0)
        _, vec = np.linalg.eigh(Xc.T @ Xc)
        Y = np.ascontiguousarray(Xc @ vec[:, -1:-3:-1])
        small = min(n, 2000)
        sharp_amd.trustworthiness(X[:small], Y[:small], n_neighbors=K)             # first call: code objects, allocations
        sharp_amd.silhouette(lab[:small], data=X[:small])
        lists = sharp_amd.knn(X, K)[0]
        rnd = random_lists(n, K, a.seed + 1)
        row = {"rows": n, "features": d, "n_neighbors": K}
        for name, fn in (("ranks_good", lambda: sharp_amd.neighbor_ranks(X, lists)),
                         ("ranks_random", lambda: sharp_amd.neighbor_ranks(X, rnd)),
                         ("ranks_d2", lambda: sharp_amd.neighbor_ranks(Y, lists))):
            r = profiled(L, fn, NR, a.reps)
            r["pairs_per_s"] = float(f"{float(n) * n / (r['nr_tile_kernel'] * 1e-3):.4g}")
            row[name] = r
        s = profiled(L, lambda: sharp_amd.silhouette(lab, data=X), ("silhouette_tiles",), a.reps)
        s["pairs_per_s"] = float(f"{float(n) * n / (s['silhouette_tiles'] * 1e-3):.4g}")
        row["silhouette"] = s
        for name in ("ranks_good", "ranks_random"):
            row[name]["ratio_to_sil_tile_kernel"] = round(row[name]["nr_tile_kernel"] / s["silhouette_tiles"], 3)
        ts = []
        for _ in range(a.reps):
            L.sharp_synchronize()
            t0 = time.perf_counter()
            score = sharp_amd.trustworthiness(X, Y, n_neighbors=K)
            ts.append((time.perf_counter() - t0) * 1e3)
        row["trustworthiness_call"] = {"min_ms": round(min(ts), 1), "score": score, "map": "first two principal components"}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
