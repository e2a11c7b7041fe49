"""Times expression_pca on synthetic Poisson counts with planted clusters and writes profiles/expr_pca_bench.json.

    python tools/bench_expr_pca.py [--shapes 50000x20000] [--rate 0.25] [--k 50]

Per shape, one run per figure after a warm-up on 2 000 cells: the whole call on a host clock, the event timers of its stages summed
over the call (expr_upload, expr_transpose, expr_stats, expr_spmm_cells, expr_spmm_genes, expr_orth, and the two product kernels alone:
expr_cells_kernel, expr_genes_kernel), and from the product kernels' own times, summed over the call's launches
  cell_side_stream_GBps   (12 bytes per stored entry + 8 l bytes per cell written) per second: what the cell side streams from HBM
  cell_side_rows_GBps     8 l bytes per stored entry per second: the rows of diag(w) Omega it reads, which stay in L2 / MALL
  gene_side_gather_GBps   8 l bytes per stored entry per second: the rows of Q the gene side gathers; the NN-descent join's measured
                          2.4 - 3.3 TB/s is the project's yardstick for such a gather
The counts are generated on the host block by block (a dense Poisson draw per 2 500 cells); 500 000 x 20 000 needs about 25 GB of host
memory and several minutes of generation and is not in the default shapes."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_louvain import profiled  # noqa: E402

STAGES = ("expr_upload", "expr_transpose", "expr_stats", "expr_spmm_cells", "expr_spmm_genes", "expr_orth", "expr_gram", "expr_cells_kernel",
          "expr_genes_kernel")
JOIN_TBPS = (2.4, 3.3)


def poisson_blocks(n, m, ncl, rate, seed, per=2500):
    """genes x cells CSC blocks of Poisson counts: gamma(0.3) base rates times `rate`, a tenth of the genes raised 3 - 8 x per cluster"""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    base = rng.gamma(0.3, size=m) * rate
    lam = np.repeat(base[:, None], ncl, axis=1)
    for c in range(ncl):
        up = rng.choice(m, m // 10, replace=False)
        lam[up, c] *= rng.uniform(3.0, 8.0, size=up.size)
    lab = rng.integers(0, ncl, size=n)
    blocks = []
    for c0 in range(0, n, per):
        blocks.append(sp.csc_matrix(rng.poisson(lam[:, lab[c0:c0 + per]]).astype(np.float64)))
    return blocks, lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="50000x20000")
    ap.add_argument("--rate", type=float, default=0.25)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--oversample", type=int, default=10)
    ap.add_argument("--n-iter", type=int, default=4)
    ap.add_argument("--ncl", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expr_pca_bench.json"))
    a = ap.parse_args()
    import sharp_amd

    sharp_amd.init(0)
    L = sharp_amd.lib()
    l = a.k + a.oversample
    rows = []
    for shape in a.shapes.split(","):
        n, m = (int(v) for v in shape.split("x"))
        blocks, lab = poisson_blocks(n, m, a.ncl, a.rate, a.seed)
        nnz = int(sum(b.nnz for b in blocks))
        sharp_amd.expression_pca(blocks[0][:, :2000], a.k, a.oversample, 1)           # first call: code objects, allocations
        fit, wall, st = profiled(L, lambda: sharp_amd.expression_pca(blocks, a.k, a.oversample, a.n_iter), STAGES)
        ck, gk = st["expr_cells_kernel"], st["expr_genes_kernel"]
        cells_ms, genes_ms = ck["ms"] / max(ck["launches"], 1), gk["ms"] / max(gk["launches"], 1)
        cols_cells = (a.n_iter + 1) * l + a.k                 # the cell side runs n_iter + 1 times with l columns and once, for the scores, with k
        cols_genes = (a.n_iter + 1) * l
        nb = sharp_amd.knn(fit["scores"][:20000], 19)
        lv = sharp_amd.louvain_snn(nb[0])
        row = {"cells": n, "genes": m, "stored_entries": nnz, "density": round(nnz / (float(n) * m), 5), "n_components": a.k, "l": l,
               "n_iter": a.n_iter, "call_ms": round(wall, 2), "stages": st,
               "cell_side_kernel_ms": round(cells_ms, 3), "gene_side_kernel_ms": round(genes_ms, 3),
               "cell_side_stream_GBps": round((12.0 * nnz * ck["launches"] + 8.0 * cols_cells * n) / (ck["ms"] * 1e-3) / 1e9, 1),
               "cell_side_rows_GBps": round(8.0 * cols_cells * nnz / (ck["ms"] * 1e-3) / 1e9, 1),
               "gene_side_gather_GBps": round(8.0 * cols_genes * nnz / (gk["ms"] * 1e-3) / 1e9, 1),
               "nn_descent_join_gather_TBps_measured": JOIN_TBPS,
               "sdev_first_last": [float(fit["sdev"][0]), float(fit["sdev"][-1])],
               "ari_louvain_snn_on_the_first_20000_cells": round(float(sharp_amd.ARI(lab[:20000] + 1, lv["membership"])["HA"]), 4),
               "runs_per_figure": 1}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
