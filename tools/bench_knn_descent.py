"""The approximate k-NN (knn_descent) against the exact search (tsne_knn) in one job, on synthetic x1 matrices of the
clustering configurations' forview outputs, as tools/bench_umap.py does for umap.  One JSON line per setting on stdout; --out collects
them in one JSON file.

    python tools/bench_knn_descent.py                                    # cfg2's and cfg3's views, K = 15 and 90
    python tools/bench_knn_descent.py --n 50000 --d 400 --K 15           # one setting
    python tools/bench_knn_descent.py --out profiles/knn_descent_bench.json

The input is prepared as visualization_SHARP prepares it (Rtsne's preparation: PCA to 50 when d > 50, normalisation).  Times come from
the library's per-kernel HIP-event timers (sharp_profile_*): tsne_knn is the exact search; knn_descent_start (projections, sorts, the
window offers), knn_descent_reverse (the sampled reverse lists of every join) and knn_descent_join (the join kernel) are the descent's.
One run per setting.  recall is the share of the exact lists' entries the descent lists hold.  join_gather_bytes_per_s counts the
candidate rows the join kernel gathered into LDS (what its filters let through: info "gathered"), 8 d bytes each, over the join
kernel's time; the microarchitecture guide's measured rate for this access pattern is 7-8 TB/s chip-wide."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_tsne import stat, synth_x1, wall  # noqa: E402

SETTINGS = [(50000, 400, 15), (50000, 400, 90), (500000, 70, 15), (500000, 70, 90)]     # cfg2's view, cfg3's view


def one(sharp_amd, L, Xp, n, d, K, a):
    from sharp_amd.tsne import _knn

    L.sharp_profile_enable(1)
    L.sharp_profile_reset()
    ei, _ = _knn(Xp, K)
    L.sharp_synchronize()
    exact_ms = stat(L, "tsne_knn")[0]
    L.sharp_profile_reset()
    (gi, _, info), wall_ms = wall(L, lambda: sharp_amd.knn_descent(Xp, K, squared=True, n_projections=a.n_projections,
                                                                    max_candidates=a.max_candidates, n_iters=a.n_iters, delta=a.delta,
                                                                    seed=a.seed, ret_info=True))
    st = {k: stat(L, k)[0] for k in ("knn_descent_start", "knn_descent_reverse", "knn_descent_join")}
    L.sharp_profile_enable(0)
    hits = 0
    for r0 in range(0, n, 8192):                                     # (blocks of rows: n x K x K booleans at once would not fit)
        hits += int((gi[r0:r0 + 8192, :, None] == ei[r0:r0 + 8192, None, :]).sum())
    dp = int(Xp.shape[1])
    descent_ms = sum(st.values())
    join_s = st["knn_descent_join"] * 1e-3
    return {"n": n, "d": d, "d_prepared": dp, "K": K, "n_projections": a.n_projections,
            "max_candidates": a.max_candidates if a.max_candidates else min(K, 30), "exact_knn_ms": round(exact_ms, 2),
            "descent_ms": round(descent_ms, 2), "start_ms": round(st["knn_descent_start"], 2), "reverse_ms": round(st["knn_descent_reverse"], 2),
            "join_ms": round(st["knn_descent_join"], 2), "descent_wall_ms": round(wall_ms, 1), "joins": info["joins"],
            "last_updates": info["updates"], "stop": info["reason"], "recall": round(hits / float(n * K), 5),
            "speedup": float(f"{exact_ms / descent_ms:.3g}") if descent_ms > 0 else None, "gathered_rows": info["gathered"],
            "join_gather_bytes_per_s": float(f"{info['gathered'] * 8.0 * dp / join_s:.4g}") if join_s > 0 else None, "runs": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--d", type=int, default=None)
    ap.add_argument("--K", type=int, default=None)
    ap.add_argument("--ncl", type=int, default=20)
    ap.add_argument("--n-projections", type=int, default=8)
    ap.add_argument("--max-candidates", type=int, default=None)
    ap.add_argument("--n-iters", type=int, default=12)
    ap.add_argument("--delta", type=float, default=0.001)
    ap.add_argument("--seed", type=int, default=10)
    ap.add_argument("--out", default=None, help="write every setting's record to this JSON file as well")
    a = ap.parse_args()
    import sharp_amd
    from sharp_amd.tsne import _prepare

    sharp_amd.init(0)
    L = sharp_amd.lib()
    settings = SETTINGS if a.n is None else [(a.n, a.d or 70, a.K or 15)]
    warm = synth_x1(2000, 70, a.ncl, 1)
    sharp_amd.knn_descent(warm, 15)                                  # first call: code objects, allocations
    sharp_amd.knn(warm, 15)
    records, prepared = [], {}
    for n, d, K in settings:
        if (n, d) not in prepared:
            prepared = {(n, d): _prepare(synth_x1(n, d, a.ncl, 1), pca=d > 50)}
        rec = one(sharp_amd, L, prepared[n, d], n, d, K, a)
        records.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:                                                    # (after every setting: a later one may be cut short)
            with open(a.out, "w") as f:
                json.dump({"tool": "tools/bench_knn_descent.py", "runs_per_setting": 1, "settings": records}, f, indent=1)


if __name__ == "__main__":
    main()
