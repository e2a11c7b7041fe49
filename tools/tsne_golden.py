"""Writes tests/golden/tsne_full_run.json: the numpy reference (tests/_tsne_ref.py) of a full 1000-iteration t-SNE run on the data
tests/test_tsne_gpu.py::test_full_run_quality uses -- too slow to recompute inside the GPU suite's time budget (minutes on one core).
    python tools/tsne_golden.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _tsne_ref as ref  # noqa: E402
from oracle import pyoracle as orc  # noqa: E402

N, M, G, NMARK, SEED = 2000, 300, 5, 40, 7


def data():
    orc.build()
    return np.log2(orc.synth_fill(SEED, M, 0, N, G, NMARK).T + 1.0)


def main():
    t0 = time.time()
    X = ref.prepare(data(), True, 50)
    P = ref.joint_p(X, 30)
    Y0 = ref.init_y(N, 2, 10, orc.runif)
    Y, costs = ref.optimise(P, Y0, max_iter=1000)
    out = {"n": N, "m": M, "G": G, "nmark": NMARK, "seed": SEED, "perplexity": 30, "max_iter": 1000, "tsne_seed": 10,
           "itercosts": costs.tolist(), "final_kl": float(costs[-1]), "seconds": time.time() - t0}
    path = os.path.join(ROOT, "tests", "golden", "tsne_full_run.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("final_kl", "seconds")}))


if __name__ == "__main__":
    main()
