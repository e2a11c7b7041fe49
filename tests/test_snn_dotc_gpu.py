"""sharp_C_snn_graph and sharp_C_louvain_snn called the way R's .C() calls a native routine (every argument a pointer into a
caller-owned vector, the status last): the plain entries' bits.  These are the calls r/sharp_hip.R makes."""
import ctypes as C

import numpy as np
import pytest

import _snn_ref as ref

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
    getattr(lib, name)(*[P(a) for a in args])


def last_error(lib):
    buf = C.create_string_buffer(b" " * 2047)
    ptr = (C.c_char_p * 1)(C.addressof(buf))
    lib.sharp_C_last_error(ptr, P(I(2048)))
    return buf.value.decode()


def test_dotc_snn_graph(sa):
    lists = ref.blobs_lists(9)[0]
    n, K = lists.shape
    want = sa.snn_graph(lists, 0.1, ret_shared=True)
    nnz = want["nnz"]
    # the count alone: col / val / shared are buffers of length 1 that are left alone
    rp, c1, v1, s1, got, st = np.zeros(n + 1), I(77), D(7.5), I(78), D(-1.0), I(-1)
    dotc(sa.lib(), "sharp_C_snn_graph", lists, D(n), I(K), D(0.1), D(0), rp, c1, v1, s1, I(0), got, st)
    assert st[0] == 0, last_error(sa.lib())
    assert got[0] == nnz and np.array_equal(rp, want["row_ptr"].astype(np.float64)) and (c1[0], v1[0], s1[0]) == (77, 7.5, 78)
    # the fill, with and without shared
    col, val, sh = np.zeros(nnz, np.int32), np.zeros(nnz), np.zeros(nnz, np.int32)
    dotc(sa.lib(), "sharp_C_snn_graph", lists, D(n), I(K), D(0.1), D(nnz), rp, col, val, sh, I(3), got, st)
    assert st[0] == 0, last_error(sa.lib())
    assert np.array_equal(col, want["col"]) and val.tobytes() == want["val"].tobytes() and np.array_equal(sh, want["shared"])
    col[:] = 0
    dotc(sa.lib(), "sharp_C_snn_graph", lists, D(n), I(K), D(0.1), D(nnz), rp, col, val, s1, I(1), got, st)
    assert st[0] == 0 and np.array_equal(col, want["col"]) and s1[0] == 78
    # a refusal arrives through the status and sharp_C_last_error, with the needed count
    dotc(sa.lib(), "sharp_C_snn_graph", lists, D(n), I(K), D(0.1), D(nnz - 1), rp, col, val, s1, I(1), got, st)
    assert st[0] != 0 and got[0] == nnz and str(nnz) in last_error(sa.lib())


def test_dotc_louvain_snn(sa):
    lists = ref.blobs_lists(19)[0]
    n, K = lists.shape
    want = sa.louvain_snn(lists, resolution=1.5, seed=3, ret_levels=True)
    mem, levels, nl, lm, st = np.zeros(n, np.int32), np.zeros(20 * 4), I(0), np.zeros(20 * n, np.int32), I(-1)
    dotc(sa.lib(), "sharp_C_louvain_snn", lists, D(n), I(K), D(ref.PRUNE), D(1.5), D(1e-7), I(20), I(200), I(4), D(3), mem, I(20), levels, nl,
         I(1), lm, st)
    assert st[0] == 0, last_error(sa.lib())
    assert np.array_equal(mem, want["membership"])
    got = [(int(r[0]), int(r[1]), int(r[2]), np.float64(r[3]).tobytes()) for r in levels.reshape(-1, 4)[:nl[0]]]
    assert got == [(l["n"], l["communities"], l["rounds"], np.float64(l["modularity"]).tobytes()) for l in want["levels"]]
    for l in range(nl[0]):
        assert np.array_equal(lm[l * n:(l + 1) * n] + 1, want["levels"][l]["membership"])
    lm1 = I(77)
    dotc(sa.lib(), "sharp_C_louvain_snn", lists, D(n), I(K), D(ref.PRUNE), D(1.5), D(1e-7), I(20), I(200), I(4), D(3), mem, I(20), levels, nl,
         I(0), lm1, st)
    assert st[0] == 0 and lm1[0] == 77 and np.array_equal(mem, want["membership"])
    dotc(sa.lib(), "sharp_C_louvain_snn", lists, D(n), I(K), D(1.5), D(1.5), D(1e-7), I(20), I(200), I(4), D(3), mem, I(20), levels, nl, I(0), lm1,
         st)
    assert st[0] != 0 and "prune must be in [0, 1]" in last_error(sa.lib())
