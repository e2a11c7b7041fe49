"""sharp_C_louvain_graph, sharp_C_louvain_neighbors and sharp_C_louvain_modularity called the way R's .C() calls a native routine (every
argument a pointer into a caller-owned vector, the status last): the plain entries' bits.  These are the calls r/sharp_hip.R makes."""
import ctypes as C

import numpy as np
import pytest

import _louvain_ref as ref

pytestmark = pytest.mark.gpu


def I(*v):
    return np.array(v, np.int32)


def D(*v):
    return np.array(v, np.float64)


def P(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


def dotc(lib, name, *args):
    fn = getattr(lib, name)
    fn(*[P(a) for a in args])


def last_error(lib):
    buf = C.create_string_buffer(b" " * 2047)
    ptr = (C.c_char_p * 1)(C.addressof(buf))
    lib.sharp_C_last_error(ptr, P(I(2048)))
    return buf.value.decode()


def levels_of(levels, nl):
    return [(int(r[0]), int(r[1]), int(r[2]), np.float64(r[3]).tobytes()) for r in levels.reshape(-1, 4)[:nl]]


def plain_levels(out):
    return [(l["n"], l["communities"], l["rounds"], np.float64(l["modularity"]).tobytes()) for l in out["levels"]]


def test_dotc_louvain_graph_and_modularity(sa):
    rp, col, val = ref.planted()[:3]
    n = len(rp) - 1
    want = sa.louvain_graph(rp, col, val, resolution=1.5, seed=3, ret_levels=True)
    mem, levels, nl, lm, st = np.zeros(n, np.int32), np.zeros(20 * 4), I(0), np.zeros(20 * n, np.int32), I(-1)
    dotc(sa.lib(), "sharp_C_louvain_graph", rp.astype(np.float64), col, val, D(n), D(1.5), D(1e-7), I(20), I(200), I(4), D(3), mem, I(20), levels,
         nl, I(1), lm, st)
    assert st[0] == 0, last_error(sa.lib())
    assert np.array_equal(mem, want["membership"]) and levels_of(levels, nl[0]) == plain_levels(want)
    for l in range(nl[0]):
        assert np.array_equal(lm[l * n:(l + 1) * n] + 1, want["levels"][l]["membership"])
    # want_levels = 0: the buffer of length 1 is left alone
    lm1 = I(77)
    dotc(sa.lib(), "sharp_C_louvain_graph", rp.astype(np.float64), col, val, D(n), D(1.5), D(1e-7), I(20), I(200), I(4), D(3), mem, I(20), levels,
         nl, I(0), lm1, st)
    assert st[0] == 0 and lm1[0] == 77 and np.array_equal(mem, want["membership"])
    Q = D(0.0)
    dotc(sa.lib(), "sharp_C_louvain_modularity", rp.astype(np.float64), col, val, D(n), (mem - 1).astype(np.int32), D(1.5), Q, st)
    assert st[0] == 0 and Q.tobytes() == np.float64(want["modularity"]).tobytes()
    # a refusal arrives through the status and sharp_C_last_error
    bad = val.copy()
    bad[0] *= 0.5
    dotc(sa.lib(), "sharp_C_louvain_graph", rp.astype(np.float64), col, bad, D(n), D(1.5), D(1e-7), I(20), I(200), I(4), D(3), mem, I(20), levels,
         nl, I(0), lm1, st)
    assert st[0] != 0 and "not symmetric" in last_error(sa.lib())


def test_dotc_louvain_neighbors(sa):
    X = np.random.default_rng(5).normal(size=(700, 8)) + 6.0 * (np.arange(700) % 4)[:, None]
    idx, dist = sa.knn(X, 10)
    n = 700
    for squared, d in ((0, dist), (1, dist ** 2)):
        want = sa.louvain_neighbors(idx, d, squared=bool(squared))
        mem, levels, nl, st = np.zeros(n, np.int32), np.zeros(20 * 4), I(0), I(-1)
        dotc(sa.lib(), "sharp_C_louvain_neighbors", idx, np.ascontiguousarray(d), D(n), I(10), I(squared), D(1.0), D(1e-7), I(20), I(200), I(4),
             D(10), mem, I(20), levels, nl, I(0), I(0), st)
        assert st[0] == 0, last_error(sa.lib())
        assert np.array_equal(mem, want["membership"]) and levels_of(levels, nl[0]) == plain_levels(want)
    assert want["n_communities"] == 4
