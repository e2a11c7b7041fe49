"""What UMAP's spectral start (init = "normlaplacian") finds and costs, next to the "pca" start in the same job.
One JSON line per run on stdout.

    python tools/bench_umap_spectral.py --n 50000 --d 400        # cfg2's view (tools/bench_umap.py's synthetic x1)
    python tools/bench_umap_spectral.py --n 500000 --d 70        # cfg3's view
    python tools/bench_umap_spectral.py --n 50000 --slab         # a connected input of that size: the solver's own cost

The input is prepared as visualization_SHARP(method="umap") prepares it.  Both starts run with n_epochs = 0, so a call is the k-NN, the
graph and the start alone.  Recorded: components, steps, residual and the outcome (0 converged, 1 not connected, 2 not converged: the
call then fell back to the "pca" start); the library's event timers umap_components (its launch count is the number of sweeps) and
umap_spectral (everything from the degrees to the residual check, host solves of T included); host:umap_init of either call (for "pca":
the download, PCA and scaling; for a converged spectral start: the scaling alone) and tsne_pca inside it.  --slab replaces the view by
points uniform in a 4 x 1.7 x 0.7 box in 10-D (tests/_umap_spectral_ref.py's slab): its graph is connected, so the solver runs to its
end whatever the views' graphs are like."""
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


def slab(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(0.0, 0.02, size=(n, 10))
    X[:, :3] += rng.uniform(0.0, 1.0, size=(n, 3)) * np.array([4.0, 1.7, 0.7])
    return X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--d", type=int, default=400)
    ap.add_argument("--ncl", type=int, default=20)
    ap.add_argument("--n-neighbors", type=int, default=15)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--slab", action="store_true", help="a connected input instead of the view")
    a = ap.parse_args()
    import sharp_amd
    from sharp_amd.tsne import _prepare

    sharp_amd.init(0)
    L = sharp_amd.lib()
    if a.slab:
        Xp, d = slab(a.n, a.seed), 10
    else:
        Xp, d = _prepare(synth_x1(a.n, a.d, a.ncl, a.seed), pca=a.d > 50), a.d
    kw = dict(n_neighbors=a.n_neighbors, n_epochs=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        sharp_amd.umap(slab(2000, 0), init="normlaplacian", **kw)   # first call: code objects, allocations
        L.sharp_profile_enable(1)
        L.sharp_profile_reset()
        _, t_pca = wall(L, lambda: sharp_amd.umap(Xp, init="pca", **kw))
        pca = {k: stat(L, k) for k in ["host:umap_init", "tsne_pca"]}
        L.sharp_profile_reset()
        out, t_nl = wall(L, lambda: sharp_amd.umap(Xp, init="normlaplacian", **kw))
        nl = {k: stat(L, k) for k in ["umap_components", "umap_spectral", "host:umap_init"]}
        L.sharp_profile_enable(0)
    info = out["init"]
    outcome = 0 if info["used"] == "normlaplacian" else 1 if info["components"] != 1 else 2
    print(json.dumps({"input": "slab" if a.slab else "view", "n": a.n, "d": d, "d_prepared": int(Xp.shape[1]), "n_neighbors": a.n_neighbors,
                      "components": info["components"], "steps": info["steps"], "residual": info["residual"], "outcome": outcome,
                      "used": info["used"], "components_ms": round(nl["umap_components"][0], 3), "sweeps": nl["umap_components"][1],
                      "spectral_ms": round(nl["umap_spectral"][0], 3), "normlaplacian_init_host_ms": round(nl["host:umap_init"][0], 3),
                      "pca_init_host_ms": round(pca["host:umap_init"][0], 3), "pca_init_pca_ms": round(pca["tsne_pca"][0], 3),
                      "call_pca_ms": round(t_pca, 1), "call_normlaplacian_ms": round(t_nl, 1)}), flush=True)


if __name__ == "__main__":
    main()
