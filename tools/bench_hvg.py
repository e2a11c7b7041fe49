"""Times highly_variable_genes and expression_pca(genes=...) on tools/bench_expr_pca.py's input and writes
profiles/hvg_bench.json.

    python tools/bench_hvg.py [--shapes 50000x20000] [--rate 0.25] [--k 50] [--n-top 2000]

Per shape, one run per figure after the same warm-up on 2 000 cells (the spread was not measured):
  * highly_variable_genes on a host clock, and the event timers of its stages in that call: expr_upload, expr_transpose, expr_stats
    (two passes over the gene-major copy), hvg_loess, hvg_clipvar (one such pass and the fold).  The yardstick of the clip pass is one
    pass of expr_stats of the same call: clipvar_over_one_stats_pass = hvg_clipvar / (expr_stats / 2).
  * the loess's weighted terms: the fit genes x the points of a local fit (about N q), and terms per second.
  * expression_pca with the selected genes beside all genes, each on a host clock with its stage timers (expr_subset among them)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_expr_pca import poisson_blocks  # noqa: E402
from bench_louvain import profiled  # noqa: E402

HVG_STAGES = ("expr_upload", "expr_transpose", "expr_stats", "hvg_loess", "hvg_clipvar")
PCA_STAGES = ("expr_upload", "expr_subset", "expr_transpose", "expr_stats", "expr_spmm_cells", "expr_spmm_genes", "expr_orth")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="50000x20000")
    ap.add_argument("--rate", type=float, default=0.25)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--oversample", type=int, default=10)
    ap.add_argument("--n-iter", type=int, default=4)
    ap.add_argument("--n-top", type=int, default=2000)
    ap.add_argument("--span", type=float, default=0.3)
    ap.add_argument("--ncl", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hvg_bench.json"))
    a = ap.parse_args()
    import sharp_amd

    sharp_amd.init(0)
    L = sharp_amd.lib()
    rows = []
    for shape in a.shapes.split(","):
        n, m = (int(v) for v in shape.split("x"))
        blocks, lab = poisson_blocks(n, m, a.ncl, a.rate, a.seed)
        nnz = int(sum(b.nnz for b in blocks))
        warm = blocks[0][:, :2000]
        sharp_amd.expression_pca(warm, a.k, a.oversample, 1)                      # first calls: code objects, allocations
        wh = sharp_amd.highly_variable_genes(warm, min(a.n_top, 200), a.span)
        sharp_amd.expression_pca(warm, 10, 5, 1, genes=wh["genes"])
        hv, hv_wall, hs = profiled(L, lambda: sharp_amd.highly_variable_genes(blocks, a.n_top, a.span), HVG_STAGES)
        fit_genes = int((hv["variances"] > 0).sum())
        terms = float(fit_genes) * hv["q"]
        sub, sub_wall, ss = profiled(L, lambda: sharp_amd.expression_pca(blocks, a.k, a.oversample, a.n_iter, genes=hv["genes"]), PCA_STAGES)
        kept = int(sum(b[hv["genes"]].nnz for b in blocks[:2])) / max(int(sum(b.nnz for b in blocks[:2])), 1)
        full, full_wall, fs = profiled(L, lambda: sharp_amd.expression_pca(blocks, a.k, a.oversample, a.n_iter), PCA_STAGES)
        one_pass = hs["expr_stats"]["ms"] / 2.0
        row = {"cells": n, "genes": m, "stored_entries": nnz, "density": round(nnz / (float(n) * m), 5), "n_top_genes": a.n_top, "span": a.span,
               "hvg_call_ms": round(hv_wall, 2), "hvg_stages": hs, "fit_genes": fit_genes, "q": hv["q"],
               "degree_counts": [int(v) for v in hv["degree_counts"]], "loess_weighted_terms": terms,
               "loess_terms_per_second": round(terms / (hs["hvg_loess"]["ms"] * 1e-3), 0),
               "one_stats_pass_ms": round(one_pass, 3), "clipvar_over_one_stats_pass": round(hs["hvg_clipvar"]["ms"] / one_pass, 2),
               "clipvar_GBps": round(8.0 * nnz / (hs["hvg_clipvar"]["ms"] * 1e-3) / 1e9, 1),
               "n_selected": hv["n_selected"], "share_of_entries_kept_first_two_blocks": round(kept, 4),
               "pca_selected_call_ms": round(sub_wall, 2), "pca_selected_stages": ss,
               "pca_all_genes_call_ms": round(full_wall, 2), "pca_all_genes_stages": fs,
               "sdev_first_selected_all": [float(sub["sdev"][0]), float(full["sdev"][0])], "runs_per_figure": 1}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
