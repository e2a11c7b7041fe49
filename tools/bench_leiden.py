"""Times leiden_neighbors next to louvain_neighbors on the neighbour graphs the maps are built from -- cfg2's and cfg3's
views of tools/bench_umap.py, prepared as tools/bench_louvain.py prepares them, n_neighbors = 15, resolution 1 -- and writes
profiles/leiden_bench.json.

    python tools/bench_leiden.py [--shapes 50000x400,500000x70] [--n-neighbors 15] [--reps 2]

Per shape, in one job, after a warm-up on 2 000 rows:
  the whole leiden_neighbors and louvain_neighbors calls on a host clock (the faster of --reps calls each; both start from host lists
  and end in a download), their stages from the event timers of the faster call (louvain_move / louvain_state / louvain_aggregate: §18's
  stages, which Leiden runs too; leiden_subtotals: the refinement's totals and flags; leiden_refine: the refine kernels of all rounds;
  leiden_split: the components inside a labelling, all levels), the levels, Q and the ARI against the generating clusters for both;
  level 0 and level 1 stage by stage, through the stage entries on the level's integer graph: the move phase from the level's start
  (louvain_move per round over the level's rounds) and then every refinement round (leiden_refine per round), so that the refine
  kernel stands next to the move kernel of the same level:
      refine_over_move       leiden_refine per round / louvain_move per round, the bar being 2
  leiden_over_louvain        the whole Leiden call / the whole Louvain call."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_louvain import profiled  # noqa: E402
from bench_tsne import synth_x1  # noqa: E402

LOUVAIN_STAGES = ("umap_graph", "umap_sym", "louvain_quantise", "louvain_move", "louvain_state", "louvain_aggregate")
LEIDEN_STAGES = LOUVAIN_STAGES + ("leiden_subtotals", "leiden_refine", "leiden_split")


def best_of(L, fn, names, reps):
    best = None
    for _ in range(reps):
        got = profiled(L, fn, names)
        if best is None or got[1] < best[1]:
            best = got
    return best


def level_stages(L, community, g, comm0, level):
    """the move phase and the refinement of one level through the stage entries: per-round kernel times"""
    (P, rounds, _), _, mv = profiled(L, lambda: community._leiden_level(*g, comm0, level=level), ("louvain_move",))
    n = len(g[0]) - 1
    sub = np.arange(n, dtype=np.int32)
    per_round = []
    for r in range(200):
        (prop, moved, wanting), _, rf = profiled(L, lambda: community._leiden_refine(*g, P, sub, level=level, rnd=r), ("leiden_refine", "leiden_subtotals"))
        if wanting == 0:
            break
        per_round.append((rf["leiden_refine"]["ms"], rf["leiden_subtotals"]["ms"], int(moved)))
        sub = prop
    move_ms = mv["louvain_move"]["ms"] / max(rounds, 1)
    refine_ms = float(np.mean([p[0] for p in per_round])) if per_round else 0.0
    row = {"level": level, "n": n, "nnz": int(g[1].size), "communities": int(np.unique(P).size), "sub_communities": int(np.unique(sub).size),
           "rounds": int(rounds), "refine_rounds": len(per_round), "move_round_ms": round(move_ms, 4), "refine_round_ms": round(refine_ms, 4),
           "refine_round_ms_first_last": [round(per_round[0][0], 4), round(per_round[-1][0], 4)] if per_round else None,
           "subtotals_round_ms": round(float(np.mean([p[1] for p in per_round])), 4) if per_round else 0.0,
           "refine_over_move": round(refine_ms / move_ms, 3) if move_ms > 0 else None}
    return row, P, sub


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="50000x400,500000x70")
    ap.add_argument("--n-neighbors", type=int, default=15)
    ap.add_argument("--ncl", type=int, default=20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leiden_bench.json"))
    a = ap.parse_args()
    import importlib

    import sharp_amd
    from sharp_amd import community
    from sharp_amd.tsne import _knn, _prepare

    um = importlib.import_module("sharp_amd.umap")
    sharp_amd.init(0)
    L = sharp_amd.lib()
    K = a.n_neighbors - 1
    rows = []
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        X = synth_x1(n, d, a.ncl, a.seed)
        truth = np.argmax(X[:, :a.ncl], axis=1)
        X = np.ascontiguousarray(_prepare(X, pca=d > 50))
        sharp_amd.leiden(X[: min(n, 2000)], n_neighbors=a.n_neighbors)                 # first calls: code objects, allocations
        sharp_amd.louvain(X[: min(n, 2000)], n_neighbors=a.n_neighbors)
        idx, d2 = _knn(X, K)
        lo, lo_wall, lo_st = best_of(L, lambda: sharp_amd.louvain_neighbors(idx, d2, squared=True), LOUVAIN_STAGES, a.reps)
        le, le_wall, le_st = best_of(L, lambda: sharp_amd.leiden_neighbors(idx, d2, squared=True), LEIDEN_STAGES, a.reps)
        ari = lambda m: round(float(sharp_amd.ARI(truth + 1, m)["HA"]), 4)   # noqa: E731
        # levels 0 and 1 stage by stage on the integer graphs
        rp, col, val = um._graph(idx, d2, squared=True)[:3]
        q = community._quantise(rp, col, val)[0]
        keep = q > 0
        row_of = np.repeat(np.arange(n), np.diff(rp))
        rp0 = np.zeros(n + 1, np.int64)
        rp0[1:] = np.cumsum(np.bincount(row_of[keep], minlength=n))
        g = (rp0, col[keep], q[keep])
        t0 = time.perf_counter()
        lev0, P, sub = level_stages(L, community, g, np.arange(n, dtype=np.int32), 0)
        per_level = [lev0]
        if lev0["sub_communities"] < n:
            crp, ccol, cq, new = community._aggregate(*g, sub)
            parent = np.zeros(len(crp) - 1, np.int32)
            parent[new[sub]] = P
            comm0 = community._leiden_split(crp, ccol, cq, parent)[0]
            per_level.append(level_stages(L, community, (crp, ccol, cq), comm0, 1)[0])
        refine_rounds = sum(l["refine_rounds"] for l in le["levels"])
        rounds = sum(l["rounds"] for l in le["levels"])
        row = {"rows": n, "features": d, "features_prepared": int(X.shape[1]), "n_neighbors": a.n_neighbors, "nnz": int(col.size),
               "leiden_call_ms": round(le_wall, 2), "louvain_call_ms": round(lo_wall, 2), "leiden_over_louvain": round(le_wall / lo_wall, 3),
               "leiden": {"stages": le_st, "levels": le["levels"], "rounds": rounds, "refine_rounds": refine_rounds,
                          "n_communities": le["n_communities"], "modularity": le["modularity"], "ari_vs_generating_clusters": ari(le["membership"]),
                          "refine_ms_per_round_all_levels": round(le_st["leiden_refine"]["ms"] / max(refine_rounds, 1), 4),
                          "move_ms_per_round_all_levels": round(le_st["louvain_move"]["ms"] / max(rounds, 1), 4),
                          "split_ms": le_st["leiden_split"]["ms"]},
               "louvain": {"stages": lo_st, "levels": lo["levels"], "rounds": sum(l["rounds"] for l in lo["levels"]),
                           "n_communities": lo["n_communities"], "modularity": lo["modularity"], "ari_vs_generating_clusters": ari(lo["membership"])},
               "per_level": per_level, "per_level_wall_s": round(time.perf_counter() - t0, 1), "reps": a.reps}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
