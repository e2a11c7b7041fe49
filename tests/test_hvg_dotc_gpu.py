"""sharp_C_expr_hvg_csc and the three sharp_C_expr_*_sub_csc entries called the way R's .C() calls a native routine (every argument a
pointer into a caller-owned vector, the status last): the plain entries' bits.  These are the calls r/sharp_hip.R makes."""
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


def test_dotc_expr_hvg(sa, blocks):
    m, top = 300, 40
    want = sa.highly_variable_genes(blocks, top, span=0.4)
    pc, ic, xc, ncb = cat(blocks)
    mu, var, ve, vn = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m)
    rank, hv, genes, ns, q, dc, st = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(top, np.int32), I(0), I(0), I(0, 0, 0), I(-1)
    dotc(sa.lib(), "sharp_C_expr_hvg_csc", pc, ic, xc, I(len(blocks)), ncb, I(m), I(top), D(0.4), mu, var, ve, vn, rank, hv, genes, ns, q, dc, st)
    assert st[0] == 0, last_error(sa.lib())
    for got, key in ((mu, "means"), (var, "variances"), (ve, "variances_expected"), (vn, "variances_norm")):
        assert got.tobytes() == want[key].tobytes(), key
    assert np.array_equal(rank, want["rank"]) and np.array_equal(hv.astype(bool), want["highly_variable"])
    assert ns[0] == want["n_selected"] == top and np.array_equal(genes, want["genes"]) and q[0] == want["q"]
    assert np.array_equal(dc, want["degree_counts"])
    dotc(sa.lib(), "sharp_C_expr_hvg_csc", pc, ic, xc, I(len(blocks)), ncb, I(m), I(top), D(1.5), mu, var, ve, vn, rank, hv, genes, ns, q, dc, st)
    assert st[0] != 0 and "highly_variable_genes: span must lie in (0, 1]" in last_error(sa.lib())
    dotc(sa.lib(), "sharp_C_expr_hvg_csc", pc, ic, xc, I(0), ncb, I(m), I(top), D(0.4), mu, var, ve, vn, rank, hv, genes, ns, q, dc, st)
    assert st[0] != 0 and "No expression data is provided" in last_error(sa.lib())


def test_dotc_expr_sub(sa, blocks):
    m, n, k = 300, 600, 6
    G = np.sort(np.random.default_rng(3).choice(m, 70, replace=False)).astype(np.int32)
    mk = G.size
    pc, ic, xc, ncb = cat(blocks)
    want = sa.expression_pca(blocks, k, oversample=4, n_iter=3, scale=True, seed=7, genes=G)
    sc, ld, sv, sdv, mu, sd, var, tv, st = np.zeros(n * k), np.zeros(mk * k), np.zeros(k), np.zeros(k), np.zeros(mk), np.zeros(mk), np.zeros(mk), D(0), I(-1)
    dotc(sa.lib(), "sharp_C_expr_pca_sub_csc", pc, ic, xc, I(len(blocks)), ncb, I(m), I(k), I(4), I(3), D(1e4), I(1), I(1), D(7), sc, ld, sv, sdv,
         mu, sd, var, tv, G, I(mk), st)
    assert st[0] == 0, last_error(sa.lib())
    for got, key in ((sc, "scores"), (ld, "loadings"), (sv, "singular_values"), (sdv, "sdev"), (mu, "center"), (sd, "scale"), (var, "gene_var")):
        assert got.tobytes() == want[key].tobytes(), key
    assert tv[0] == want["total_var"]
    # *n_genes = 0: all genes, the bits of the plain entry
    full = sa.expression_pca(blocks, k, oversample=4, n_iter=3, scale=True, seed=7)
    sc2, ld2, mu2, sd2, var2 = np.zeros(n * k), np.zeros(m * k), np.zeros(m), np.zeros(m), np.zeros(m)
    dotc(sa.lib(), "sharp_C_expr_pca_sub_csc", pc, ic, xc, I(len(blocks)), ncb, I(m), I(k), I(4), I(3), D(1e4), I(1), I(1), D(7), sc2, ld2, sv, sdv,
         mu2, sd2, var2, tv, I(0), I(0), st)
    assert st[0] == 0, last_error(sa.lib())
    assert sc2.tobytes() == full["scores"].tobytes() and ld2.tobytes() == full["loadings"].tobytes()
    # the statistics and the transform
    ws = sa.gene_stats(blocks, genes=G)
    smu, svar, snnz, cs = np.zeros(mk), np.zeros(mk), np.zeros(mk), np.zeros(n)
    dotc(sa.lib(), "sharp_C_expr_stats_sub_csc", pc, ic, xc, I(len(blocks)), ncb, I(m), D(1e4), I(1), smu, svar, snnz, cs, G, I(mk), st)
    assert st[0] == 0, last_error(sa.lib())
    assert smu.tobytes() == ws["mean"].tobytes() and svar.tobytes() == ws["var"].tobytes() and cs.tobytes() == ws["cell_sum"].tobytes()
    assert np.array_equal(snnz, ws["nnz"].astype(np.float64))
    out = np.zeros(n * k)
    dotc(sa.lib(), "sharp_C_expr_pca_transform_sub_csc", pc, ic, xc, I(len(blocks)), ncb, I(m), D(1e4), I(1), want["loadings"], want["center"],
         want["scale"], I(k), out, G, I(mk), st)
    assert st[0] == 0, last_error(sa.lib())
    assert out.tobytes() == sa.expression_pca_transform(blocks, want).tobytes()
    bad = G.copy()
    bad[3] = bad[2]
    dotc(sa.lib(), "sharp_C_expr_stats_sub_csc", pc, ic, xc, I(len(blocks)), ncb, I(m), D(1e4), I(1), smu, svar, snnz, cs, bad, I(mk), st)
    assert st[0] != 0 and "gene_stats: genes holds a gene twice (position 3, counted from 0)" in last_error(sa.lib())
