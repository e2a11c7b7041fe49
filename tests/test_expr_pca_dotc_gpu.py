"""sharp_C_expr_pca_csc, sharp_C_expr_stats_csc and sharp_C_expr_pca_transform_csc called the way R's .C() calls a native routine (every
argument a pointer into a caller-owned vector, the status last): the plain entries' bits.  These are the calls r/sharp_hip.R makes."""
import ctypes as C

import numpy as np
import pytest

import _expr_pca_ref as ref

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


def cat(blocks):
    """the blocks' @p / @i / @x one after the other, and their cells as doubles"""
    return (np.concatenate([np.asarray(b.indptr, np.int32) for b in blocks]), np.concatenate([np.asarray(b.indices, np.int32) for b in blocks] + [I()]),
            np.concatenate([np.asarray(b.data, np.float64) for b in blocks] + [D()]), D(*[b.shape[1] for b in blocks]))


@pytest.fixture(scope="module")
def blocks():
    return ref.ragged(ref.planted(600, 300, 4)[0], [0, 250, 251])


def test_dotc_expr_pca(sa, blocks):
    m, n, k = 300, 600, 8
    want = sa.expression_pca(blocks, k, oversample=4, n_iter=3, scale=True, seed=7)
    pc, ic, xc, ncb = cat(blocks)
    sc, ld, sv, sdv, mu, sd, var, tv, st = np.zeros(n * k), np.zeros(m * k), np.zeros(k), np.zeros(k), np.zeros(m), np.zeros(m), np.zeros(m), D(0), I(-1)
    dotc(sa.lib(), "sharp_C_expr_pca_csc", pc, ic, xc, I(len(blocks)), ncb, I(m), I(k), I(4), I(3), D(1e4), I(1), I(1), D(7), sc, ld, sv, sdv, mu,
         sd, var, tv, st)
    assert st[0] == 0, last_error(sa.lib())
    for got, key in ((sc, "scores"), (ld, "loadings"), (sv, "singular_values"), (sdv, "sdev"), (mu, "center"), (sd, "scale"), (var, "gene_var")):
        assert got.tobytes() == want[key].tobytes(), key
    assert tv[0] == want["total_var"]
    dotc(sa.lib(), "sharp_C_expr_pca_csc", pc, ic, xc, I(len(blocks)), ncb, I(m), I(125), I(4), I(3), D(1e4), I(1), I(1), D(7), sc, ld, sv, sdv,
         mu, sd, var, tv, st)
    assert st[0] != 0 and "n_components + oversample must be <= 128" in last_error(sa.lib())
    dotc(sa.lib(), "sharp_C_expr_pca_csc", pc, ic, xc, I(0), ncb, I(m), I(k), I(4), I(3), D(1e4), I(1), I(1), D(7), sc, ld, sv, sdv, mu, sd, var,
         tv, st)
    assert st[0] != 0 and "No expression data is provided" in last_error(sa.lib())


def test_dotc_expr_stats_and_transform(sa, blocks):
    m, n, k = 300, 600, 5
    pc, ic, xc, ncb = cat(blocks)
    want = sa.gene_stats(blocks)
    mu, var, nnz, cs, st = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(n), I(-1)
    dotc(sa.lib(), "sharp_C_expr_stats_csc", pc, ic, xc, I(len(blocks)), ncb, I(m), D(1e4), I(1), mu, var, nnz, cs, st)
    assert st[0] == 0, last_error(sa.lib())
    assert mu.tobytes() == want["mean"].tobytes() and var.tobytes() == want["var"].tobytes() and cs.tobytes() == want["cell_sum"].tobytes()
    assert np.array_equal(nnz, want["nnz"].astype(np.float64))
    fit = sa.expression_pca(blocks, k)
    sc = np.zeros(n * k)
    dotc(sa.lib(), "sharp_C_expr_pca_transform_csc", pc, ic, xc, I(len(blocks)), ncb, I(m), D(1e4), I(1), fit["loadings"], fit["center"],
         fit["scale"], I(k), sc, st)
    assert st[0] == 0, last_error(sa.lib())
    assert sc.tobytes() == sa.expression_pca_transform(blocks, fit).tobytes()
    bad = xc.copy()
    bad[3] = -1.0
    dotc(sa.lib(), "sharp_C_expr_stats_csc", pc, ic, bad, I(len(blocks)), ncb, I(m), D(1e4), I(1), mu, var, nnz, cs, st)
    assert st[0] != 0 and "gene_stats: a negative value under normalize_total / log1p (cell 0, counted from 0)" in last_error(sa.lib())
