"""What a diffusion map finds and costs on the benchmarked inputs, next to the exact k-NN of the same job and to the
spectral start's solver on the same graph.  One JSON record per run, printed and merged into --out (profiles/diffmap_bench.json).

    python tools/bench_diffmap.py --n 50000 --d 400        # cfg2's view (tools/bench_umap.py's synthetic x1): 20 components
    python tools/bench_diffmap.py --n 500000 --d 70        # cfg3's view
    python tools/bench_diffmap.py --n 50000 --slab         # a connected input of that size
    python tools/bench_diffmap.py --n 500000 --slab

One job after a warm-up on 2 000 rows.  Settings: n_neighbors 15, n_comps 15, the default tol.  Recorded: components, the solved
component's size, steps (operator applications), restarts and the outcome; the six event timers; the whole diffmap_neighbors call and
the exact k-NN on a host clock.  Yardsticks: the time of one Lanczos step against one step of umap_spectral on the solved component (the
kernels are the same; umap_spectral's timer also holds its degrees, host solves and residual check); the rotation against the bytes it
must move, n (m + p) 8, and the residual pass against nnz 12 + n k 16, both over the chip's 5.4 TB/s stream ceiling
(profiles/r03_copy_bandwidth.txt).  diffmap_restart also times the upload of S and H and the copy of one column, so a rotation's own
time is below it."""
import argparse
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_tsne import stat, synth_x1, wall  # noqa: E402
from bench_umap_spectral import slab  # noqa: E402

STREAM_BYTES_PER_MS = 5.4e12 / 1e3
TIMERS = ["diffmap_transitions", "diffmap_extract", "diffmap_lanczos", "diffmap_restart", "diffmap_residuals", "dpt"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--d", type=int, default=400)
    ap.add_argument("--ncl", type=int, default=20)
    ap.add_argument("--n-neighbors", type=int, default=15)
    ap.add_argument("--n-comps", type=int, default=15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--slab", action="store_true", help="a connected input instead of the view")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffmap_bench.json"))
    a = ap.parse_args()
    import sharp_amd
    from sharp_amd.tsne import _prepare
    from sharp_amd.umap import _graph, _spectral

    sharp_amd.init(0)
    L = sharp_amd.lib()
    Xp = slab(a.n, a.seed) if a.slab else _prepare(synth_x1(a.n, a.d, a.ncl, a.seed), pca=a.d > 50)
    K = a.n_neighbors - 1
    k = a.n_comps - 1
    m, p = 2 * (8 * ((k + k // 2 + 8) // 8)) + 16, 8 * ((k + k // 2 + 8) // 8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        warm = sharp_amd.diffmap(slab(2000, 0), n_neighbors=a.n_neighbors, n_comps=a.n_comps)   # first call: code objects, allocations
        sharp_amd.dpt(warm, root=0)
        L.sharp_profile_enable(1)
        L.sharp_profile_reset()
        (idx, dist), t_knn = wall(L, lambda: sharp_amd.knn(Xp, K))
        knn_ms = stat(L, "tsne_knn")[0]
        L.sharp_profile_reset()
        dm, t_call = wall(L, lambda: sharp_amd.diffmap_neighbors(idx, dist, n_comps=a.n_comps))
        root = int(np.flatnonzero(dm["in_component"])[0])
        _, t_dpt = wall(L, lambda: sharp_amd.dpt(dm, root=root))
        tm = {name: stat(L, name) for name in TIMERS}
        # the spectral start's solver on the solved component (it refuses a graph in pieces), the same job
        rp, col, val = _graph(idx, dist)[:3]
        if dm["components"] > 1:
            from sharp_amd.diffmap import _component

            rp, col, val = _component(rp, col, val, a.n_comps)[2]
        L.sharp_profile_reset()
        sp = _spectral(rp, col, val, dims=3)
        sp_ms = stat(L, "umap_spectral")[0]
        L.sharp_profile_enable(0)
    ns, nnz = int(dm["component_size"]), int(col.size)
    steps, rot = dm["steps"], tm["diffmap_restart"][1]
    lan_step = tm["diffmap_lanczos"][0] / max(steps, 1)
    sp_step = sp_ms / max(sp["steps"], 1)
    rot_ms = tm["diffmap_restart"][0] / max(rot, 1)
    rot_floor = ns * (m + p) * 8 / STREAM_BYTES_PER_MS
    res_ms = tm["diffmap_residuals"][0] / max(tm["diffmap_residuals"][1], 1)
    res_floor = (nnz * 12 + ns * k * 16) / STREAM_BYTES_PER_MS
    rec = {"input": "slab" if a.slab else "view", "n": a.n, "d_prepared": int(Xp.shape[1]), "n_neighbors": a.n_neighbors, "n_comps": a.n_comps,
           "m": m, "p": p, "components": int(dm["components"]), "component_size": ns, "component_nnz": nnz, "steps": steps,
           "restarts": int(dm["restarts"]), "outcome": 0 if dm["converged"] else 2, "largest_residual": float(dm["residual"].max()),
           "timers_ms": {name: round(v[0], 3) for name, v in tm.items()}, "timer_scopes": {name: int(v[1]) for name, v in tm.items()},
           "call_diffmap_neighbors_ms": round(t_call, 1), "call_dpt_ms": round(t_dpt, 2), "call_knn_ms": round(t_knn, 1),
           "tsne_knn_ms": round(knn_ms, 3),
           "lanczos_step_ms": round(lan_step, 4), "umap_spectral_steps": int(sp["steps"]), "umap_spectral_outcome": int(sp["outcome"]),
           "umap_spectral_ms": round(sp_ms, 3), "umap_spectral_step_ms": round(sp_step, 4), "lanczos_step_ratio": round(lan_step / sp_step, 3),
           "rotation_scope_ms": round(rot_ms, 4), "rotation_floor_ms": round(rot_floor, 4), "rotation_ratio": round(rot_ms / rot_floor, 2),
           "residual_pass_ms": round(res_ms, 4), "residual_floor_ms": round(res_floor, 4), "residual_ratio": round(res_ms / res_floor, 2)}
    print(json.dumps(rec), flush=True)
    runs = []
    if os.path.exists(a.out):
        runs = [r for r in json.load(open(a.out)) if (r["input"], r["n"]) != (rec["input"], rec["n"])]
    runs.append(rec)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(sorted(runs, key=lambda r: (r["input"], r["n"])), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
