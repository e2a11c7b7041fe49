"""sharp_C_leiden_graph, sharp_C_leiden_neighbors and sharp_C_leiden_snn called the way R's .C() calls a native routine (every argument a
pointer into a caller-owned vector, the status last): the plain entries' bits.  These are the calls r/sharp_hip.R makes."""
import numpy as np
import pytest

import _louvain_ref as ref
from test_louvain_dotc_gpu import D, I, dotc, last_error

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


def levels_of(levels, nl):
    return [tuple(int(x) for x in r[:5]) + (np.float64(r[5]).tobytes(),) for r in levels.reshape(-1, 6)[:nl]]


def plain_levels(out):
    return [(l["n"], l["communities"], l["sub_communities"], l["rounds"], l["refine_rounds"], np.float64(l["modularity"]).tobytes())
            for l in out["levels"]]


def test_dotc_leiden_graph(sa):
    rp, col, val = ref.planted()[:3]
    n = len(rp) - 1
    want = sa.leiden_graph(rp, col, val, resolution=1.5, seed=3, max_refine_rounds=50, ret_levels=True)
    mem, Q, levels, nl, lm, st = np.zeros(n, np.int32), D(0.0), np.zeros(20 * 6), I(0), np.zeros(20 * n, np.int32), I(-1)
    dotc(sa.lib(), "sharp_C_leiden_graph", rp.astype(np.float64), col, val, D(n), D(1.5), D(1e-7), I(20), I(200), I(4), I(50), D(3), mem, Q, I(20),
         levels, nl, I(1), lm, st)
    assert st[0] == 0, last_error(sa.lib())
    assert np.array_equal(mem, want["membership"]) and levels_of(levels, nl[0]) == plain_levels(want)
    assert Q.tobytes() == np.float64(want["modularity"]).tobytes()
    for l in range(nl[0]):
        assert np.array_equal(lm[l * n:(l + 1) * n] + 1, want["levels"][l]["membership"])
    # want_levels = 0: the buffer of length 1 is left alone
    lm1 = I(77)
    dotc(sa.lib(), "sharp_C_leiden_graph", rp.astype(np.float64), col, val, D(n), D(1.5), D(1e-7), I(20), I(200), I(4), I(50), D(3), mem, Q, I(20),
         levels, nl, I(0), lm1, st)
    assert st[0] == 0 and lm1[0] == 77 and np.array_equal(mem, want["membership"])
    # a refusal arrives through the status and sharp_C_last_error
    dotc(sa.lib(), "sharp_C_leiden_graph", rp.astype(np.float64), col, val, D(n), D(1.5), D(1e-7), I(20), I(200), I(4), I(0), D(3), mem, Q, I(20),
         levels, nl, I(0), lm1, st)
    assert st[0] != 0 and "max_refine_rounds must be in 1 .. 100000" in last_error(sa.lib())


def test_dotc_leiden_neighbors_and_snn(sa):
    X = np.random.default_rng(5).normal(size=(700, 8)) + 6.0 * (np.arange(700) % 4)[:, None]
    idx, dist = sa.knn(X, 10)
    n = 700
    for squared, d in ((0, dist), (1, dist ** 2)):
        want = sa.leiden_neighbors(idx, d, squared=bool(squared))
        mem, Q, levels, nl, st = np.zeros(n, np.int32), D(0.0), np.zeros(20 * 6), I(0), I(-1)
        dotc(sa.lib(), "sharp_C_leiden_neighbors", idx, np.ascontiguousarray(d), D(n), I(10), I(squared), D(1.0), D(1e-7), I(20), I(200), I(4),
             I(200), D(10), mem, Q, I(20), levels, nl, I(0), I(0), st)
        assert st[0] == 0, last_error(sa.lib())
        assert np.array_equal(mem, want["membership"]) and levels_of(levels, nl[0]) == plain_levels(want)
        assert Q.tobytes() == np.float64(want["modularity"]).tobytes()
    assert want["n_communities"] == 4
    want = sa.leiden_snn(idx, 0.1, resolution=0.5, seed=2)
    mem, Q, levels, nl, st = np.zeros(n, np.int32), D(0.0), np.zeros(20 * 6), I(0), I(-1)
    dotc(sa.lib(), "sharp_C_leiden_snn", idx, D(n), I(10), D(0.1), D(0.5), D(1e-7), I(20), I(200), I(4), I(200), D(2), mem, Q, I(20), levels, nl,
         I(0), I(0), st)
    assert st[0] == 0, last_error(sa.lib())
    assert np.array_equal(mem, want["membership"]) and levels_of(levels, nl[0]) == plain_levels(want)
    assert Q.tobytes() == np.float64(want["modularity"]).tobytes()
