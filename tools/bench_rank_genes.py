"""Times rank_genes_groups on the input of tools/bench_expr_pca.py (synthetic Poisson counts with planted clusters, the
planted clusters as the groups) and writes profiles/rank_genes_bench.json.

    python tools/bench_rank_genes.py [--shape 50000x20000] [--rate 0.25] [--ncl 20]

After a warm-up on 2 000 cells, one run per figure: the call on a host clock for "rest" and for a reference group, for both methods, with
the library's event timers per stage (load + transform: expr_upload + expr_transpose + expr_stats; ordering: rank_genes_order;
statistics: rank_genes_stats; reference kernel with its sort and scan: rank_genes_ref; per-group sort: rank_genes_sort), and
get_marker_genes_unlimited on the same blocks and labels in the same job.  Two yardsticks:
  (a) the statistics kernel against the time the chip's 5.4 TB/s stream ceiling (profiles/r03_copy_bandwidth.txt) needs for the bytes it
      must read and write: 12 bytes per stored entry (the key and the group), 16 G bytes per chunk (the chunk's sums per group) and 16
      bytes per (group, gene) of integer results
  (b) the whole "rest" call against get_marker_genes_unlimited, the existing code doing the nearest job
Each is "inside" the bar when within twice the yardstick, "outside" otherwise."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_expr_pca import poisson_blocks  # noqa: E402
from bench_louvain import profiled  # noqa: E402

STAGES = ("expr_upload", "expr_transpose", "expr_stats", "rank_genes_order", "rank_genes_stats", "rank_genes_ref", "rank_genes_sort")
STREAM_TBPS = 5.4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="50000x20000")
    ap.add_argument("--rate", type=float, default=0.25)
    ap.add_argument("--ncl", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_genes_bench.json"))
    a = ap.parse_args()
    import sharp_amd
    from sharp_amd import expr_pca

    sharp_amd.init(0)
    L = sharp_amd.lib()
    n, m = (int(v) for v in a.shape.split("x"))
    blocks, lab = poisson_blocks(n, m, a.ncl, a.rate, a.seed)
    nnz = int(sum(b.nnz for b in blocks))
    chunk = expr_pca._row_caps()[0]
    per_gene = np.zeros(m, np.int64)
    for b in blocks:
        per_gene += np.bincount(b.indices, minlength=m)
    nch = int(((per_gene + chunk - 1) // chunk).sum())
    G = int(np.unique(lab).size)
    warm = blocks[0][:, :2000]
    for method in ("wilcoxon", "t-test"):
        sharp_amd.rank_genes_groups(warm, lab[:2000], method=method)                 # first calls: code objects, allocations
        sharp_amd.rank_genes_groups(warm, lab[:2000], method=method, reference=0)
    sharp_amd.get_marker_genes_unlimited([warm], {"pred_clusters": lab[:2000] + 1})
    calls = {}
    for method in ("wilcoxon", "t-test"):
        for ref in ("rest", 0):
            _, wall, st = profiled(L, lambda: sharp_amd.rank_genes_groups(blocks, lab, method=method, reference=ref), STAGES)
            calls[f"{method}/{ref}"] = {"call_ms": round(wall, 2), "stages": st,
                                        "load_ms": round(sum(st[k]["ms"] for k in ("expr_upload", "expr_transpose", "expr_stats")), 3)}
            print(json.dumps({f"{method}/{ref}": calls[f"{method}/{ref}"]}), flush=True)
    t0 = time.perf_counter()
    sharp_amd.get_marker_genes_unlimited(blocks, {"pred_clusters": lab + 1})
    marker_ms = (time.perf_counter() - t0) * 1e3
    stats_ms = calls["wilcoxon/rest"]["stages"]["rank_genes_stats"]["ms"]
    need_bytes = 12.0 * nnz + 16.0 * G * nch + 16.0 * G * m
    floor_ms = need_bytes / (STREAM_TBPS * 1e12) * 1e3
    rest_ms = calls["wilcoxon/rest"]["call_ms"]
    row = {"cells": n, "genes": m, "stored_entries": nnz, "groups": G, "chunks": nch, "calls": calls,
           "a_statistics_kernel_ms": stats_ms, "a_bytes": need_bytes, "a_stream_floor_ms_at_5.4TBps": round(floor_ms, 3),
           "a_ratio": round(stats_ms / floor_ms, 2), "a_verdict": "inside" if stats_ms <= 2 * floor_ms else "outside",
           "b_rest_call_ms": rest_ms, "b_get_marker_genes_unlimited_ms": round(marker_ms, 2), "b_ratio": round(rest_ms / marker_ms, 2),
           "b_verdict": "inside" if rest_ms <= 2 * marker_ms else "outside", "runs_per_figure": 1}
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(row, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
