"""Times scrublet on the input of tools/bench_expr_pca.py and writes profiles/doublets_bench.json.

    python tools/bench_doublets.py [--shape 50000x20000] [--rate 0.25] [--ratio 2] [--out profiles/doublets_bench.json]

One run per figure, after the same warm-up on 2 000 cells.  The variable genes and the PCA of the observed cells are fitted first and timed
on a host clock; the call with that fit (pca=) is then run under the library's event timers: doublet_count, doublet_scan, doublet_fill,
doublet_transform (the transform and the gene subset) and doublet_product per slab, summed over the slabs, the k-NN on the n + n_sim
rows (doublet_knn) and the neighbour counts; the call itself and the default call (which fits on its own) on a host clock.
The yardstick of the synthesis: the count pass reads 4 bytes and the fill pass 12 bytes per parent entry, and the fill writes 12 bytes
per stored entry of a doublet; at the chip's 5.4 TB/s stream ceiling (profiles/r03_copy_bandwidth.txt) that is synth_yardstick_ms.  The
project's bar is twice that time."""
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

STAGES = ("expr_upload", "doublet_count", "doublet_scan", "doublet_fill", "doublet_transform", "expr_subset", "doublet_product", "expr_cells_kernel",
          "doublet_knn", "doublet_neighbor_counts")
STREAM_TBPS = 5.4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="50000x20000")
    ap.add_argument("--rate", type=float, default=0.25)
    ap.add_argument("--ratio", type=float, default=2.0)
    ap.add_argument("--ncl", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--skip-default-call", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "doublets_bench.json"))
    a = ap.parse_args()
    import sharp_amd
    from sharp_amd import doublets

    sharp_amd.init(0)
    L = sharp_amd.lib()
    n, m = (int(v) for v in a.shape.split("x"))
    blocks, _ = poisson_blocks(n, m, a.ncl, a.rate, a.seed)
    nnz = int(sum(b.nnz for b in blocks))
    sharp_amd.scrublet(blocks[0][:, :2000], sim_doublet_ratio=a.ratio)          # first call: code objects, allocations
    t0 = time.perf_counter()
    hv = sharp_amd.highly_variable_genes(blocks, 2000)
    pc = sharp_amd.expression_pca(blocks, 30, genes=hv["genes"], scale=True)
    fit_ms = (time.perf_counter() - t0) * 1e3
    r, wall, st = profiled(L, lambda: sharp_amd.scrublet(blocks, sim_doublet_ratio=a.ratio, pca=pc), STAGES)
    length = np.concatenate([np.diff(b.indptr) for b in blocks]).astype(np.int64)
    parent_entries = int(length[r["parents"]].sum())
    # the doublets' stored entries, from the genes two parents share: counted on the host for a sample, since the slabs stay on the device
    sample = r["parents"][:2000]
    sim = doublets.simulate_doublets(blocks, parents=sample)
    out_entries = int(round(sim["counts"].nnz / float(length[sample].sum()) * parent_entries))
    yard_ms = (16.0 * parent_entries + 12.0 * out_entries) / (STREAM_TBPS * 1e12) * 1e3
    synth_ms = st["doublet_count"]["ms"] + st["doublet_fill"]["ms"]
    row = {"cells": n, "genes": m, "stored_entries": nnz, "sim_doublet_ratio": a.ratio, "n_sim": r["n_sim"], "n_neighbors": r["n_neighbors"],
           "k_adj": r["k_adj"], "slabs": st["doublet_fill"]["launches"], "parent_entries": parent_entries,
           "doublet_entries_estimated_from_2000": out_entries, "fit_hvg_pca_ms": round(fit_ms, 1), "call_with_fit_ms": round(wall, 1),
           "stages": st, "synth_count_plus_fill_ms": round(synth_ms, 3), "synth_yardstick_ms": round(yard_ms, 3),
           "synth_over_yardstick": round(synth_ms / yard_ms, 2), "bar": 2.0, "stream_ceiling_TBps": STREAM_TBPS,
           "threshold": r["threshold"], "threshold_found": r["threshold_found"], "runs_per_figure": 1}
    if not a.skip_default_call:
        t0 = time.perf_counter()
        sharp_amd.scrublet(blocks, sim_doublet_ratio=a.ratio)
        row["default_call_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump({"rows": [row]}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
