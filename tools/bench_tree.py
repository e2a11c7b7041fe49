"""Times dist, the agglomeration, HCASS2 and the whole plot_markers call at 2 000, 10 000 and 16 384 cells x 100 and 400
markers, next to the CPU path (scipy pdist + the oracle's hclust) on the same box, and writes profiles/hclust_tree_bench.json.

    python tools/bench_tree.py [--sizes 2000,10000,16384] [--markers 100,400] [--reps 3] [--no-cpu]

GPU times: a synchronised host clock around each call (every entry ends in a download), after one warm-up call; min / median of --reps.
Stage times (dist kernel, agglomeration kernels, HCASS2) come from the library's profile table in a separate profiled call; one more
profiled call with method = "centroid" times the sequential kernel, which ward.D only takes on exact ties."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": round(min(ts), 2), "median_ms": round(statistics.median(ts), 2)}


def stat(L, name):
    ms, k = C.c_double(), C.c_longlong()
    L.sharp_profile_get(name.encode(), C.byref(ms), C.byref(k))
    return round(ms.value, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,10000,16384")
    ap.add_argument("--markers", default="100,400")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hclust_tree_bench.json"))
    a = ap.parse_args()
    import sharp_amd

    sharp_amd.init(0)
    L = sharp_amd.lib()
    rows = []
    for n in [int(v) for v in a.sizes.split(",")]:
        for p in [int(v) for v in a.markers.split(",")]:
            rng = np.random.default_rng(n + p)
            lab = np.sort(rng.integers(1, 11, n))
            x = rng.normal(size=(n, p)) + rng.normal(size=(10, p))[lab - 1]      # cells x markers, ten clusters
            row = {"cells": n, "markers": p}
            row["dist"] = timed(lambda: sharp_amd.dist(x), a.reps)
            row["hclust_fused"] = timed(lambda: sharp_amd.hclust(x=x), a.reps)
            L.sharp_profile_enable(1)
            L.sharp_profile_reset()
            sharp_amd.hclust(x=x)
            L.sharp_synchronize()
            row["stages_ms"] = {k: stat(L, k) for k in ("dist", "row_prep", "hclust", "hclust_sequential", "host:hcass2")}
            L.sharp_profile_reset()
            t0 = time.perf_counter()
            sharp_amd.hclust(x=x, method="centroid")                             # not reducible: always the one-workgroup sequential kernel
            row["hclust_fused_centroid_sequential_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            L.sharp_synchronize()
            row["sequential_kernel_ms"] = stat(L, "hclust_sequential")
            L.sharp_profile_enable(0)
            sg = {"mginfo": {"gene": np.arange(p), "icluster": np.repeat(np.arange(1, 11), -(-p // 10))[:p], "auc": rng.random(p),
                             "pvalue": rng.random(p) * 1e-3}, "mat": np.ascontiguousarray(x.T), "label": lab, "logmark": False}
            f = os.path.join(tempfile.gettempdir(), "bench_tree_heatmap.png")
            row["plot_markers_no_figure"] = timed(lambda: sharp_amd.plot_markers(sg, N_marker=p, nratio=1.0, plot=False), a.reps)
            row["plot_markers_with_png"] = timed(lambda: sharp_amd.plot_markers(sg, N_marker=p, nratio=1.0, filename=f, filetype="png"), 1)
            if not a.no_cpu:
                from scipy.spatial.distance import pdist

                from oracle import pyoracle as orc

                t0 = time.perf_counter()
                d = pdist(x)
                t1 = time.perf_counter()
                orc.hclust(d, n, "ward.D")
                t2 = time.perf_counter()
                row["cpu_pdist_ms"] = round((t1 - t0) * 1e3, 1)
                row["cpu_oracle_hclust_ms"] = round((t2 - t1) * 1e3, 1)
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
