"""Per-stage timing of umap_transform (new rows placed in a fitted UMAP map) on a synthetic x1 matrix shaped like cfg3's
view: a reference of --n-ref rows, --n-query new rows transformed in blocks of --block, n_neighbors 15.  One JSON line per block on
stdout, then a summary line; --out writes all of them to a JSON file (profiles/umap_transform_bench.json).

    python tools/bench_umap_transform.py                                   # 500 000 x 50 reference, 500 000 queries in blocks of 50 000
    python tools/bench_umap_transform.py --n-ref 50000 --n-query 100000    # a smaller run

The model's map is NOT a fitted one: Y_ref is the reference's first two columns mapped onto [0, 10], which costs nothing and gives the
epoch kernel positions of a map's scale -- its time depends on the number of slots, (1 + negative_sample_rate) n_neighbors per row, not
on where the rows lie.  Stages come from the library's HIP-event timers (sharp_profile_*): umap_knn_cross (centring, knn_cross_kernel,
the merge), umap_tr_weights, umap_tr_epochs; block_ms is the whole call on a synchronised host clock (uploads and downloads included).
pairs_per_s counts candidate pairs, block rows x n_ref; tsne_knn_pairs_per_s is Rtsne's self k-NN (n_ref x n_ref, K = n_neighbors - 1)
timed in the same process on the same GPU, for comparison.  No figure here is asserted anywhere."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_tsne import stat, synth_x1, wall  # noqa: E402

STAGES = ("umap_knn_cross", "umap_tr_weights", "umap_tr_epochs")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ref", type=int, default=500000)
    ap.add_argument("--n-query", type=int, default=500000)
    ap.add_argument("--block", type=int, default=50000)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--ncl", type=int, default=20)
    ap.add_argument("--n-neighbors", type=int, default=15)
    ap.add_argument("--negative-sample-rate", type=int, default=5)
    ap.add_argument("--fit-epochs", type=int, default=200, help="the fit's epochs (a transform runs a third of them)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-self-knn", action="store_true", help="skip the tsne_knn comparison")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sharp_amd
    from sharp_amd.tsne import _knn

    sharp_amd.init(0)
    L = sharp_amd.lib()
    X = synth_x1(a.n_ref + a.n_query, a.d, a.ncl, a.seed)
    Xr, Xq = np.ascontiguousarray(X[: a.n_ref]), X[a.n_ref:]
    y = Xr[:, :2]
    Y_ref = (y - y.min(0)) / (y.max(0) - y.min(0)) * 10.0
    ab = sharp_amd.umap_ab(1.0, 0.01)
    lines = []
    with sharp_amd.UmapModel(Xr[:2000], Y_ref[:2000], a.n_neighbors, ab[0], ab[1], 6) as warm:   # first call: code objects, allocations
        sharp_amd.umap_transform(Xq[:500], warm)
    model, t_model = wall(L, lambda: sharp_amd.UmapModel(Xr, Y_ref, a.n_neighbors, ab[0], ab[1], a.fit_epochs))
    L.sharp_profile_enable(1)
    for b0 in range(0, a.n_query, a.block):
        blk = np.ascontiguousarray(Xq[b0: b0 + a.block])
        L.sharp_profile_reset()
        out, t = wall(L, lambda: sharp_amd.umap_transform(blk, model, negative_sample_rate=a.negative_sample_rate, row_offset=b0))
        st = {k: stat(L, k)[0] for k in STAGES}
        lines.append({"block": b0 // a.block, "rows": int(blk.shape[0]), "n_ref": a.n_ref, "d": a.d, "n_neighbors": a.n_neighbors,
                      "n_epochs": out["n_epochs"], "knn_cross_ms": round(st["umap_knn_cross"], 3), "weights_ms": round(st["umap_tr_weights"], 3),
                      "epochs_ms": round(st["umap_tr_epochs"], 3), "block_ms": round(t, 2),
                      "pairs_per_s": float(f"{blk.shape[0] * a.n_ref / (st['umap_knn_cross'] * 1e-3):.4g}")})
        print(json.dumps(lines[-1]), flush=True)
    summary = {"summary": True, "n_ref": a.n_ref, "n_query": a.n_query, "block": a.block, "d": a.d, "model_create_ms": round(t_model, 1),
               "knn_cross_ms": round(sum(v["knn_cross_ms"] for v in lines), 2), "weights_ms": round(sum(v["weights_ms"] for v in lines), 2),
               "epochs_ms": round(sum(v["epochs_ms"] for v in lines), 2), "blocks_wall_ms": round(sum(v["block_ms"] for v in lines), 1),
               "pairs_per_s": float(f"{a.n_query * a.n_ref / (sum(v['knn_cross_ms'] for v in lines) * 1e-3):.4g}")}
    model.close()
    if not a.no_self_knn:
        L.sharp_profile_reset()
        _knn(Xr, a.n_neighbors - 1)
        L.sharp_synchronize()
        ms = stat(L, "tsne_knn")[0]
        summary["tsne_knn_ms"] = round(ms, 2)
        summary["tsne_knn_pairs_per_s"] = float(f"{a.n_ref * a.n_ref / (ms * 1e-3):.4g}")
    L.sharp_profile_enable(0)
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"blocks": lines, "summary": summary}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
