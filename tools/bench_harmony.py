"""Times harmony_integrate on cfg2's and cfg3's views of tools/bench_umap.py -- the synthetic x1 of 50 000 x 400 and of
500 000 x 70, prepared to 50 columns as visualization_SHARP prepares them -- with 4 and 10 batches assigned at random and a planted
offset per batch (a Gaussian direction of twice the columns' mean standard deviation), and writes profiles/harmony_bench.json.

    python tools/bench_harmony.py [--shapes 50000x400:4,500000x70:10] [--k 100] [--reps 2]

Per shape, after a warm-up on 2 000 rows:
  * the whole call (defaults, n_clusters = --k) on a host clock with the profile off, the faster of --reps calls ("call_ms"); then
    the same call with the event timers on, again the faster of --reps ("call_profiled_ms"), and that call's timers: harmony_init
    (whose span also holds the host's hashing, layout and partial sort between its two events), harmony_assign, harmony_sums,
    harmony_objective, harmony_correct.  Their "launches" count timer scopes, not kernel launches.
  * per clustering round: the event time (assign + sums + objective over all rounds / the rounds), and "launches_per_round_from_code":
    not counted by any profiler but read off csrc/harmony.hip as DESIGN.md §23 lists them, 3 per block that holds a cell + 8 (+ 1 per
    further 65 535 slabs), and one copy of the objective to the host
  * the assign kernel alone over one full pass (the stage entry's event timer, the faster of --reps), its bytes -- 8 (K + d) a cell, a
    read + write stream -- per second, and the ratio to bytes / 5.4 TB/s (profiles/r03_copy_bandwidth.txt's ceiling for such a stream)
  * the share of a cell's 30 nearest neighbours in its own batch before and after, on 2 000 sampled cells (exact k-NN on the host)"""
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

STAGES = ("harmony_init", "harmony_assign", "harmony_sums", "harmony_objective", "harmony_correct")
CEILING = 5.4e12


def same_batch_share(Z, batch, sample, k=30):
    q = Z[sample]
    D = (q * q).sum(axis=1)[:, None] + (Z * Z).sum(axis=1)[None] - 2.0 * q @ Z.T
    D[np.arange(sample.size), sample] = np.inf
    nn = np.argpartition(D, k, axis=1)[:, :k]
    return float((batch[nn] == batch[sample][:, None]).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="50000x400:4,500000x70:10")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--ncl", type=int, default=20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harmony_bench.json"))
    a = ap.parse_args()
    import sharp_amd
    from sharp_amd import harmony
    from sharp_amd.tsne import _prepare

    sharp_amd.init(0)
    L = sharp_amd.lib()
    rows = []
    for shape in a.shapes.split(","):
        dims, B = shape.split(":")
        n, d0 = (int(v) for v in dims.split("x"))
        B = int(B)
        rng = np.random.default_rng(a.seed)
        X = np.ascontiguousarray(_prepare(synth_x1(n, d0, a.ncl, a.seed), pca=d0 > 50))
        d = X.shape[1]
        batch = rng.integers(0, B, n)
        off = rng.standard_normal((B, d))
        off *= 2.0 * X.std(axis=0).mean() / np.sqrt((off * off).sum(axis=1, keepdims=True))
        Z = np.ascontiguousarray(X + off[batch])
        sharp_amd.harmony_integrate(Z[:2000], batch[:2000], n_clusters=min(a.k, 60), max_iter=1, max_iter_cluster=2)      # code objects, allocations
        plain = []
        for _ in range(a.reps):
            L.sharp_synchronize()
            t0 = time.perf_counter()
            sharp_amd.harmony_integrate(Z, batch, n_clusters=a.k)
            plain.append((time.perf_counter() - t0) * 1e3)
        best = None
        for _ in range(a.reps):
            out, wall, st = profiled(L, lambda: sharp_amd.harmony_integrate(Z, batch, n_clusters=a.k), STAGES)
            if best is None or wall < best[1]:
                best = (out, wall, st)
        out, wall, st = best
        rounds = int(out["rounds"].sum())
        round_ms = (st["harmony_assign"]["ms"] + st["harmony_sums"]["ms"] + st["harmony_objective"]["ms"]) / max(rounds, 1)
        # one full assign pass alone, on the call's own result
        Zh = out["Z_corr"] / np.sqrt((out["Z_corr"] ** 2).sum(axis=1, keepdims=True))
        P = np.ones((B, a.k))
        ms = []
        for _ in range(a.reps):
            _, _, sa_ = profiled(L, lambda: harmony._assign(Zh, out["Y"], batch, P, 0.1), ("harmony_assign",))
            ms.append(sa_["harmony_assign"]["ms"])
        pass_ms = min(ms)
        nbytes = 8.0 * (a.k + d) * n
        sample = rng.choice(n, 2000, replace=False)
        row = {"rows": n, "features": d0, "features_prepared": d, "batches": B, "n_clusters": a.k, "call_ms": round(min(plain), 2),
               "call_profiled_ms": round(wall, 2), "stages": st,
               "n_iter": out["n_iter"], "rounds": [int(v) for v in out["rounds"]], "converged": out["converged"],
               "objective": [float(v) for v in out["objective"]], "round_event_ms": round(round_ms, 4),
               "launches_per_round_from_code": 3 * 20 + 8,                      # (every one of the 20 blocks holds cells at these sizes)
               "assign_pass_ms": round(pass_ms, 4), "assign_pass_bytes": nbytes, "assign_pass_TBps": round(nbytes / (pass_ms * 1e-3) / 1e12, 3),
               "assign_pass_over_stream_floor": round(pass_ms * 1e-3 / (nbytes / CEILING), 2),
               "same_batch_share_before": round(same_batch_share(Z, batch, sample), 4),
               "same_batch_share_after": round(same_batch_share(out["Z_corr"], batch, sample), 4), "chance": round(1.0 / B, 4), "reps": a.reps}
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump({"rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
