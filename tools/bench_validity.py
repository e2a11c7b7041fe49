"""Times silhouette() and calinski_harabasz() at the sizes a user runs -- the views SHARP returns for cfg2 (50 000 x 50)
and cfg3 (500 000 x 50) and plot_markers' largest matrix (16 384 x 400), k = 12 -- and writes profiles/validity_bench.json.

    python tools/bench_validity.py [--shapes 50000x50,500000x50,16384x400] [--reps 3] [--no-cpu] [--cpu-max 50000]

Call times: a host clock around each call (every entry ends in a download), after one warm-up call; min / median of --reps.  Kernel
times come from the library's event timers in a separate profiled call.  The fp64 operations are counted from the shapes: n^2 pairs x
p features x 3 (subtract, multiply, add; euclidean) or x 2 (one fused multiply-add; correlation).  The vector peak of 78.6 TFLOP/s
counts a fused multiply-add as two operations per lane and clock; the euclidean loop issues three separate instructions per pair and
feature, so its bound is instruction issue at half that figure, and both shares are reported.  Beside each GPU figure: sklearn's
silhouette_samples on the same box (up to --cpu-max cells), and at n <= 16 384 the route through dist() + silhouette(d=)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_VECTOR_F64 = 78.6e12


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
    ap.add_argument("--shapes", default="50000x50,500000x50,16384x400")
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-max", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validity_bench.json"))
    a = ap.parse_args()
    import sharp_amd

    sharp_amd.init(0)
    L = sharp_amd.lib()
    rows = []
    for shape in a.shapes.split(","):
        n, p = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(n + p)
        lab = rng.integers(1, a.k + 1, n)
        x = rng.normal(size=(n, p)) + rng.normal(scale=3, size=(a.k, p))[lab - 1]
        moved = rng.random(n) < 0.05
        lab[moved] = rng.integers(1, a.k + 1, int(moved.sum()))
        row = {"cells": n, "features": p, "clusters": int(np.unique(lab).size)}
        for distance, ops in (("euclidean", 3), ("correlation", 2)):
            r = {"call": timed(lambda: sharp_amd.silhouette(lab, data=x, distance=distance), a.reps)}
            L.sharp_profile_enable(1)
            L.sharp_profile_reset()
            sharp_amd.silhouette(lab, data=x, distance=distance)
            L.sharp_synchronize()
            r["kernels_ms"] = {k: stat(L, k) for k in ("silhouette_unit_rows", "silhouette_tiles", "silhouette_finish")}
            L.sharp_profile_enable(0)
            flops = float(n) * n * p * ops
            sec = r["kernels_ms"]["silhouette_tiles"] / 1e3
            r["fp64_ops_counted"] = flops
            r["tile_kernel_tflops"] = round(flops / sec / 1e12, 2)
            r["share_of_vector_peak"] = round(flops / sec / PEAK_VECTOR_F64, 3)
            if distance == "euclidean":                            # three instructions where the peak counts one FMA as two operations
                r["share_of_issue_bound"] = round(flops / sec / (PEAK_VECTOR_F64 / 2), 3)
            row["silhouette_" + distance] = r
        for kind in ("euclidean", "1-corr"):
            row["calinski_harabasz_" + kind] = timed(lambda: sharp_amd.calinski_harabasz(x, lab, distance=kind), a.reps)
        if n <= 16384:
            row["dist_then_silhouette_d"] = timed(lambda: sharp_amd.silhouette(lab, d=sharp_amd.dist(x)), a.reps)
            L.sharp_profile_enable(1)
            L.sharp_profile_reset()
            sharp_amd.silhouette(lab, d=sharp_amd.dist(x))
            L.sharp_synchronize()
            row["dist_then_silhouette_d_kernels_ms"] = {k: stat(L, k) for k in ("dist", "dist_condense", "silhouette_dist")}
            L.sharp_profile_enable(0)
        if a.no_cpu or n > a.cpu_max:
            row["cpu_sklearn_silhouette_samples_ms"] = "not measured"
        else:
            from sklearn.metrics import calinski_harabasz_score, silhouette_samples

            t0 = time.perf_counter()
            silhouette_samples(x, lab)
            t1 = time.perf_counter()
            calinski_harabasz_score(x, lab)
            t2 = time.perf_counter()
            row["cpu_sklearn_silhouette_samples_ms"] = round((t1 - t0) * 1e3, 1)
            row["cpu_sklearn_calinski_harabasz_ms"] = round((t2 - t1) * 1e3, 1)
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
