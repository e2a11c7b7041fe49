"""sharp_C_rank_genes_csc called the way R's .C() calls a native routine (every argument a pointer into a caller-owned vector, the status
last): the plain entry's bits, and its status and message on a refusal.  This is the call r/sharp_hip.R makes."""
import ctypes as C

import numpy as np
import pytest

import _expr_pca_ref as ref

pytestmark = pytest.mark.gpu
_F = ("scores", "pvals", "pvals_adj", "logfoldchanges", "auc", "means", "means_ref", "pct", "pct_ref")


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


def last_error(lib):
    buf = C.create_string_buffer(b" " * 2047)
    ptr = (C.c_char_p * 1)(C.addressof(buf))
    lib.sharp_C_last_error(ptr, P(I(2048)))
    return buf.value.decode()


def test_dotc_rank_genes(sa):
    X, lab = ref.planted(600, 300, 4)[:2]
    blocks = ref.ragged(X, [250])
    codes = np.asarray(lab, np.int32) - int(np.min(lab))
    G, m, top = int(codes.max()) + 1, 300, 25
    keep = np.arange(0, 300, 3, dtype=np.int32)
    mk = keep.size
    want = sa.rank_genes_groups(blocks, codes, method="t-test", reference=1, genes=keep, n_genes=top)
    pc = np.concatenate([np.asarray(b.indptr, np.int32) for b in blocks])
    ic = np.concatenate([np.asarray(b.indices, np.int32) for b in blocks])
    xc = np.concatenate([np.asarray(b.data, np.float64) for b in blocks])
    ncb = D(*[b.shape[1] for b in blocks])
    out = {k: np.zeros(G * mk) for k in _F}
    gs, order, st = np.zeros(G), np.zeros(G * top, np.int32), I(-1)

    def call(n_groups, method):
        getattr(sa.lib(), "sharp_C_rank_genes_csc")(*[P(a) for a in (pc, ic, xc, I(len(blocks)), ncb, I(m), codes, I(n_groups), I(method), I(1),
                                                                      D(1e4), I(1), keep, I(mk), I(1), I(0), I(top), gs, *[out[k] for k in _F],
                                                                      order, st)])

    call(G, 1)
    assert st[0] == 0, last_error(sa.lib())
    for k in _F:
        assert out[k].tobytes() == want[k].tobytes(), k
    assert np.array_equal(gs, want["group_sizes"].astype(np.float64)) and np.array_equal(order.reshape(G, top), want["order"])
    call(G, 2)
    assert st[0] != 0 and "rank_genes_groups: method must be 0 (wilcoxon) or 1 (t-test)" in last_error(sa.lib())
    call(G + 1, 0)
    assert st[0] != 0 and "has no cell" in last_error(sa.lib())
