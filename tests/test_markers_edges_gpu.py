"""GPU tests of get_marker_genes' per-gene pass (sharp_amd/csrc/markers.hip) where its launches and its sort change regime: a second gene
tile, more than 16 cells per workgroup, the sparse kernels' grid-stride loop, every path of the segmented sort, hundreds of clusters, the
planted edges of the rank arithmetic, and every C entry and layout.  Every comparison is against tests/_markers_ref.py (pinned on the CPU by
tests/test_markers_cpu.py), cross-checked against the oracle; no case compares one path of the library with another as its only check.

What _check asserts for EVERY gene: the same cluster; sparsity bitwise; auc within rtol 1e-12 / atol 1e-14; p within rtol 1e-9 above
1e-290, <= 1e-289 where the reference is at or below 1e-290, NaN where it is NaN; FC within the bound of _markers_ref.fc_bound (2^-51 for
whole-number genes).  The cluster comparison has no exceptions: two distinct mean ranks differ by at least 2 / n^2 while the kernel's
carry about n 2^-52 of rounding, and for ng > 1 the reference's second-best AUROC is either the same rational as the best (the first
tried must win) or more than 1e-9 below it -- both asserted on the reference before anything is compared.

The segmented sort: rocPRIM 4.2.0 (ROCm 7.2.0), default_segmented_radix_sort_config for an 8-byte integer key without values.  Its
gfx942 entry is kernel_config<256, 8> = 2048 items per block with WarpSortConfig<8, 4, 256, 64, 16, 8, 256>: partitioning_threshold 64,
warp sorts up to 32 and 128 items.  This rocPRIM has no gfx950 entry, so on the MI355X the generic one applies: kernel_config<128, 17> =
2176 items per block, WarpSortConfig<32, 4, 256, 3000, 32, 4, 256>: partitioning_threshold 3000, warp sort up to 128 items.  A segment
longer than the block's items takes the multi-pass path; fewer segments than the threshold take the unpartitioned path.  The planted
lengths stand on each side of 32, 64, 128, 256, 2048 and 2176, so either table is covered."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import _markers_ref as R

pytestmark = pytest.mark.gpu

STAGES = (b"marker_count", b"marker_fill", b"marker_sort", b"marker_stats")


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


# ---- the cases and their references: built once, shared, never modified ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(name):
    t0 = time.time()
    if name.startswith("many"):
        built = R.case_many_clusters(int(name[4:]))
    else:
        built = getattr(R, "case_" + name)()
    X, label, G = built[:3]
    X.setflags(write=False)
    label.setflags(write=False)
    print("case %s: built in %.2f s" % (name, time.time() - t0))
    return built


@functools.lru_cache(maxsize=None)
def _ref(name, theta, ng):
    X, label, G = _case(name)[:3]
    t0 = time.time()
    pre = _pre(name)
    tab, info = R.marker_stats(X, label, G, theta=theta, ng=ng, pre=pre)
    print("reference %s ng = %d: %.2f s" % (name, ng, time.time() - t0))
    return tab, info


@functools.lru_cache(maxsize=None)
def _pre(name):
    X, label, G = _case(name)[:3]
    t0 = time.time()
    pre = R.rank_sums(X, label, G)
    print("reference ranks %s: %.2f s" % (name, time.time() - t0))
    return pre


# ---- calling the C entries ---------------------------------------------------------------------------------------------------------------

def _err(sa):
    e = sa.lib().sharp_last_error()
    return e.decode() if isinstance(e, bytes) else str(e)


def _dense(sa, X, label, G, theta, ng):
    """sharp_marker_genes on the (genes, cells) matrix, column-major with ld = m"""
    from sharp_amd._lib import f64, i32

    m, n = X.shape
    Xf = np.asfortranarray(X, dtype=np.float64)
    lab = np.ascontiguousarray(label, np.int32)
    out = np.full((m, 5), -7.0)
    rc = sa.lib().sharp_marker_genes(f64(Xf), m, n, m, i32(lab), G, theta, ng, f64(out))
    assert rc == 0, _err(sa)
    return out


def _stored(X, extra=None):
    """(genes, cells) -> scipy csc of the non-zeros, plus explicitly STORED entries wherever `extra` is set (zeros stay stored)"""
    import scipy.sparse as sp

    mask = X != 0
    if extra is not None:
        mask = mask | extra
    r, c = np.nonzero(mask)
    return sp.csc_matrix((X[r, c], (r, c)), shape=X.shape)


def _csc(sa, slots, m, label, G, theta, ng, expect_ok=True):
    """sharp_marker_genes_blocks_csc.  slots: per block (colptr view of ncells + 1 int32, rowidx base, val base, ncells): the row indices
    and values are addressed from the arrays' START by colptr, as the slots of one larger dgCMatrix are"""
    from sharp_amd._lib import f64, i32, i64

    B = len(slots)
    keep = [(np.asarray(cp), np.ascontiguousarray(ri, np.int32), np.ascontiguousarray(vx, np.float64)) for cp, ri, vx, _ in slots]
    for cp, _, _ in keep:
        assert cp.dtype == np.int32 and cp.flags.c_contiguous
    cpp = (C.c_void_p * B)(*[k[0].ctypes.data for k in keep])
    rip = (C.c_void_p * B)(*[k[1].ctypes.data for k in keep])
    vxp = (C.c_void_p * B)(*[k[2].ctypes.data for k in keep])
    ncb = np.array([s[3] for s in slots], np.int64)
    lab = np.ascontiguousarray(label, np.int32)
    out = np.full((m, 5), -7.0)
    rc = sa.lib().sharp_marker_genes_blocks_csc(cpp, rip, vxp, i64(ncb), B, m, i32(lab), G, theta, ng, f64(out))
    if expect_ok:
        assert rc == 0, _err(sa)
    return (out if expect_ok else rc)


def _csc_whole(sa, X, label, G, theta, ng, extra=None):
    a = _stored(X, extra)
    return _csc(sa, [(a.indptr.astype(np.int32), a.indices, a.data, X.shape[1])], X.shape[0], label, G, theta, ng)


# ---- the comparison ----------------------------------------------------------------------------------------------------------------------

def _premises(info, n, ng, what):
    mm = info["mr_margin"]
    nzm = mm[(mm > 0) & np.isfinite(mm)]
    noise = 64 * n * 2.0 ** -52
    assert 1.0 / (2.0 * n * n) > noise and (nzm.size == 0 or nzm.min() > 1.0 / (2.0 * n * n)), (what, nzm.min())
    assert np.array_equal(info["mr_tie"], (mm == 0.0))
    if ng > 1:
        bad = ~(info["auc_tie"] | (info["auc_margin"] > 1e-9))
        assert not bad.any(), (what, "AUROC near-tie in the seeded input: change the seed", np.flatnonzero(bad), info["auc_margin"][bad])


def _check(out, tab, info, n, ng, what):
    _premises(info, n, ng, what)
    assert np.array_equal(out[:, 1], tab[:, 1]), (what, "icluster", np.flatnonzero(out[:, 1] != tab[:, 1])[:10])
    assert np.array_equal(out[:, 3], tab[:, 3]), (what, "sparsity", np.flatnonzero(out[:, 3] != tab[:, 3])[:10])
    print(what, "max |auc - reference|", np.abs(out[:, 0] - tab[:, 0]).max())
    np.testing.assert_allclose(out[:, 0], tab[:, 0], rtol=1e-12, atol=1e-14, err_msg=what)
    p, pr = out[:, 2], tab[:, 2]
    nan = np.isnan(pr)
    assert np.array_equal(np.isnan(p), nan), (what, "NaN p-values", np.flatnonzero(np.isnan(p) != nan))
    big = ~nan & (pr > 1e-290)
    tiny = ~nan & ~big
    print(what, "p: max relative", (np.abs(p[big] - pr[big]) / pr[big]).max() if big.any() else None, "rows at or below 1e-290:", int(tiny.sum()))
    np.testing.assert_allclose(p[big], pr[big], rtol=1e-9, atol=0, err_msg=what)
    assert np.all(p[tiny] <= 1e-289) and np.all(p[tiny] >= 0), (what, p[tiny])
    fc, fr = out[:, 4], tab[:, 4]
    bound = R.fc_bound(tab, info)
    fin = np.isfinite(bound)
    assert np.all(bound[fin & info["counts"]] == 2.0 ** -51)
    rel = np.abs(fc[fin] - fr[fin]) / np.abs(fr[fin])
    print(what, "FC: max relative", rel.max() if fin.any() else None, "max of difference / bound", (rel / bound[fin]).max() if fin.any() else None,
          "largest bound", bound[fin].max() if fin.any() else None)
    assert np.all(rel <= bound[fin]), (what, "FC", np.flatnonzero(fin)[rel > bound[fin]][:10])
    assert np.array_equal(fc[~fin], fr[~fin], equal_nan=True), (what, "FC (inf / 0 rows)")


def _check_oracle(oracle, out, X, label, G, theta, ng, genes, info, tab, what):
    """the oracle's rows of `genes` (at least 64, or all of them): icluster, sparsity, and the existing test's tolerances"""
    genes = np.asarray(genes)
    assert genes.size >= min(64, X.shape[0])
    ref = oracle.marker_genes(np.ascontiguousarray(X[genes]), label, G, theta=theta, ng=ng)
    o = out[genes]
    assert np.array_equal(o[:, 1], ref[:, 1]) and np.array_equal(o[:, 3], ref[:, 3]), what
    np.testing.assert_allclose(o[:, 0], ref[:, 0], rtol=1e-12, atol=1e-14, err_msg=what)
    nan = np.isnan(ref[:, 2])
    ok = ~nan & (ref[:, 2] > 1e-290)
    np.testing.assert_allclose(o[ok, 2], ref[ok, 2], rtol=1e-9, err_msg=what)
    assert np.array_equal(np.isnan(o[:, 2]), nan), what
    bound = R.fc_bound(tab, info)[genes]
    fin = np.isfinite(bound)
    assert np.all(np.abs(o[fin, 4] - ref[fin, 4]) <= (bound[fin] + 1e-13) * np.abs(ref[fin, 4])), what    # (1e-13: the oracle's own sum)
    assert np.array_equal(o[~fin, 4], ref[~fin, 4], equal_nan=True), what


def _same_but_fc(a, b, what):
    """bitwise equal in auc, icluster, pvalue, sparsity.  FC alone may differ between two calls (and between the dense and the sparse
    form): a cluster's sum of values is an LDS atomic sum of doubles, whose order changes from run to run; every other column comes from
    integer atomics (rank sums, counts, tie term) and from arithmetic on them in one thread"""
    assert np.array_equal(a[:, :4], b[:, :4], equal_nan=True), (what, np.flatnonzero((a[:, :4] != b[:, :4]).any(1))[:10])


def _full_case(sa, oracle, name, theta, ngs, oracle_genes, extra=None):
    X, label, G = _case(name)[:3]
    m, n = X.shape
    for ng in ngs:
        tab, info = _ref(name, theta, ng)
        d = _dense(sa, X, label, G, theta, ng)
        _check(d, tab, info, n, ng, "%s dense ng = %d" % (name, ng))
        s = _csc_whole(sa, X, label, G, theta, ng, extra)
        _check(s, tab, info, n, ng, "%s csc ng = %d" % (name, ng))
        _same_but_fc(d, s, name + " dense against csc")
        _check_oracle(oracle, d, X, label, G, theta, ng, oracle_genes, info, tab, "%s oracle ng = %d" % (name, ng))
    _same_but_fc(d, _dense(sa, X, label, G, theta, ngs[-1]), name + " twice")
    _same_but_fc(s, _csc_whole(sa, X, label, G, theta, ngs[-1], extra), name + " csc twice")
    return d


# ---- gene tiles --------------------------------------------------------------------------------------------------------------------------

def test_two_gene_tiles(sa, oracle):
    """m = 16384 + 37, n = 600, G = 4: blockIdx.y = 1 runs, with a ragged tile width gn = 37, through sharp_marker_genes and
    sharp_marker_genes_blocks_csc.  Able to fail: gene 16383 (last of tile 0) is dense without a zero, gene 16384 (first of tile 1) is all
    zero, gene m - 1 has three non-zeros.  If g0 were dropped from the row pointer X + c * ld + g0, tile 1 would count genes 0..36 again:
    gene 16384 would come back with gene 0's sparsity instead of 0 and gene m - 1 with gene 36's instead of 3 / 600.  If g0 were dropped
    from counts[g0 + q], the counts of genes 16384.. would land on genes 0..36: gene m - 1 would read sparsity 0 and gene 36 too much.  A
    gn taken as MG_TILE in tile 1 would read past gene m - 1 into the next cell's genes and raise counts beyond m (every gene of the
    tile is compared, so a shifted row cannot pass either)."""
    X, label, G = _case("two_tiles")
    m, n = X.shape
    pick = np.r_[0:40, 16370:16400, m - 20:m]
    d = _full_case(sa, oracle, "two_tiles", 1e-4, (1, 4), pick)
    assert d[16384].tolist() == [0.0, 0.0, 1.0, 0.0, 0.0] and d[16383, 3] == 1.0 and d[m - 1, 3] == 3 / n


def test_exactly_one_full_tile(sa, oracle):
    """m = 16384, n = 64, G = 2: gn == MG_TILE and a grid of ONE tile -- (m + MG_TILE - 1) / MG_TILE must not become 2, and the last gene
    of the tile (three non-zeros) must be written.  Whole-number counts, so every gene has ties and the normal approximation applies."""
    X, label, G = _case("full_tile")
    d = _full_case(sa, oracle, "full_tile", 1e-4, (1, 2), np.r_[0:40, 16384 - 40:16384])
    assert d[16383, 3] == 3 / 64 and d[0].tolist() == [0.0, 0.0, 1.0, 0.0, 0.0]


def test_front_ends_on_two_tiles(sa, tmp_path):
    """get_marker_genes, get_marker_genes_unlimited (dense list, sparse list) and get_marker_genes_unlimited2 (three gene-wise block
    files of 5000 / 6000 / 5421 genes) on the two-tile input: selection, Holm adjustment and ordering done in numpy from the reference
    table; and device.marker_genes_dev on a non-contiguous dX[:, :m] view against sharp_marker_genes"""
    import scipy.sparse as sp
    import torch
    from sharp_amd import blocks as sblocks
    from sharp_amd import device

    X, label, G = _case("two_tiles")
    m, n = X.shape
    names = np.array(["g%d" % i for i in range(m)])
    y = {"pred_clusters": np.asarray(label)}

    def select(tab, theta, auc, pvalue, fc=None):
        sel = (tab[:, 3] > theta) & ~np.isnan(tab[:, 2])
        idx = np.flatnonzero(sel)
        padj = R.holm(tab[sel, 2])
        adauc = min(auc, min(tab[sel, 0][tab[sel, 1] == c].max() for c in np.unique(tab[sel, 1])))
        # premise: no gene stands within the arithmetic of a threshold, so the library's own last bits cannot change the selection
        assert adauc == auc and np.abs(tab[sel, 0] - auc).min() > 1e-9 and np.abs(padj - pvalue).min() > 1e-9 * pvalue
        assert fc is None or np.abs(tab[sel, 4] - fc).min() > 1e-9
        pick = (padj < pvalue) & (tab[sel, 0] > adauc)
        if fc is not None:
            pick &= tab[sel, 4] >= fc
        return idx[pick], padj[pick], idx

    # get_marker_genes: theta = 1e-4, ng = 4, ordered by (icluster, -FC, -auc, p, -sparsity)
    tab, _ = _ref("two_tiles", 1e-4, 4)
    res = sa.get_marker_genes(X, y, ng=4, gene_names=names)
    idx, padj, allidx = select(tab, 1e-4, 0.7, 0.01, fc=2)
    order = np.lexsort((-tab[idx, 3], padj, -tab[idx, 0], -tab[idx, 4], tab[idx, 1]))
    assert idx.size > 100 and res["mginfo"]["gene"].tolist() == names[idx[order]].tolist()
    assert np.array_equal(res["mginfo"]["icluster"], tab[idx[order], 1].astype(np.int64))
    np.testing.assert_allclose(res["mginfo"]["pvalue"], padj[order], rtol=1e-9)
    assert res["gallinfo"]["gene"].tolist() == names[allidx].tolist()
    assert np.array_equal(res["mat"], X[idx[order]])
    assert any(g > 16384 for g in idx) and any(g < 16384 for g in idx)       # markers from both tiles

    # get_marker_genes_unlimited: theta = 1e-5, ng = 1, cells in three ragged blocks
    tab1, _ = _ref("two_tiles", 1e-5, 1)
    cuts = [0, 250, 400, n]
    dense = [X[:, cuts[b]:cuts[b + 1]] for b in range(3)]
    nonzero = tab1[:, 3] > 0
    t = tab1[nonzero]
    idx1, _, _ = select(t, 1e-5, 0.85, 0.01)
    want = names[nonzero][idx1]
    for r in (sa.get_marker_genes_unlimited(dense, y, gene_names=names),
              sa.get_marker_genes_unlimited([sp.csr_matrix(b) for b in dense], y, gene_names=names)):
        assert want.size > 100 and r["mginfo"]["gene"].tolist() == want.tolist()
        assert np.array_equal(r["mat"], X[[int(g[1:]) for g in want]]) and np.array_equal(r["label"], label)
    assert "g16384" not in want.tolist()

    # get_marker_genes_unlimited2: gene-wise files, ng = min(10, G) = 4, p < 0.05
    d = tmp_path / "genes"
    d.mkdir()
    gcuts = [0, 5000, 11000, m]
    for i in range(3):
        sblocks.write_block(str(d / ("part%d.blk" % (i + 1))), X[gcuts[i]:gcuts[i + 1]])
    tab4, _ = _ref("two_tiles", 1e-5, 4)
    r2 = sa.get_marker_genes_unlimited2(str(d), y)
    idx2, padj2, all2 = select(tab4, 1e-5, 0.85, 0.05)
    file_of = np.searchsorted(gcuts, idx2, side="right")
    assert idx2.size > 100 and r2["mginfo"]["gene"].tolist() == ["part%d.blk:%d" % (f, g - gcuts[f - 1]) for f, g in zip(file_of, idx2)]
    np.testing.assert_allclose(r2["mginfo"]["auc"], tab4[idx2, 0], rtol=1e-12)
    assert np.array_equal(r2["mginfo"]["icluster"], tab4[idx2, 1].astype(np.int64)) and r2["gallinfo"]["gene"].size == all2.size

    # the resident entry on a view: rows of m + 6 floats, the first m are the genes; the padding holds values that must not be read
    host = np.full((n, m + 6), 99.0, np.float32)
    host[:, :m] = X.T
    dX = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    view = dX[:, :m]
    assert not view.is_contiguous() and view.stride(0) == m + 6
    got = device.marker_genes_dev(view, label, G, theta=1e-4, ng=4)
    _check(got, tab, _ref("two_tiles", 1e-4, 4)[1], n, 4, "marker_genes_dev on a view")
    _same_but_fc(got, _dense(sa, X, label, G, 1e-4, 4), "marker_genes_dev against sharp_marker_genes")


# ---- long lists: cells per workgroup, the grid-stride loop, the sort ---------------------------------------------------------------------

def test_long_lists_few_genes(sa, oracle):
    """m = 48, n = 20011, G = 6, dense and csc.  Dense: cells_per_block = ceil(20011 / (4 x 256 CUs)) = 20, and 20011 = 1000 x 20 + 11, a
    ragged last chunk (c1 = min(n, ...)); a chunk taken whole would read 9 cells past the matrix and count them, so sparsities would be
    off.  csc: 16 x 256 workgroups of four waves are 16384 waves for 20011 cells, so 3627 waves run the loop body twice; a loop run once
    drops cells 16384.. and every long gene's sparsity falls short.  The sort: 48 segments are below partitioning_threshold (64 in the
    gfx942 table, 3000 in the generic one this rocPRIM uses on gfx950: see the module docstring), so the unpartitioned path runs; genes
    0..21 have lists of LONG_LENGTHS = 0, 1, 2, 3, 31..33, 63..65, 127..129, 255..257 (warp sort / single block, either table),
    2047..2049 and 2175..2177 (the last length one block sorts, and the first it cannot, in the gfx942 and the generic table); genes 22
    and 24 have no zero at all (n items, t0 == 0), 23 has n - 1, 25..28 have 5000, 10000, 4353 and 2304: multi-pass in either table.  A
    list left unsorted or sorted on the low word shifts ranks, so auc and the cluster of these continuous genes would differ."""
    X, label, G = _case("long_lists")
    d = _full_case(sa, oracle, "long_lists", 1e-5, (1, 6), np.arange(48))
    nz = np.count_nonzero(X, axis=1)
    assert np.array_equal(d[:, 3], nz / 20011.0) and d[0].tolist() == [0.0, 0.0, 1.0, 0.0, 0.0] and d[22, 3] == 1.0


def test_long_lists_many_genes(sa, oracle):
    """m = 3000, n = 9001, G = 6, a tenth of the genes dense (a third of those without any zero): 3000 segments reach the generic
    table's partitioning_threshold (3000) and pass the gfx942 one (64), so the partitioned path sorts the same long segments: 300 lists
    of about 7200..9001 items go to the large-segment kernel in several passes, lists of 2176 / 2177 and 2048 / 2049 items stand on each
    side of one block's items, 128 / 129 on each side of the warp sort, and the ~450-item lists of the sparse genes go to the single-block
    sort.  The oracle checks the first 128 genes, which hold every planted one."""
    _full_case(sa, oracle, "long_many", 1e-5, (1, 6), np.arange(128))


# ---- clusters ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", [256, 257, 1024])
def test_many_clusters(sa, oracle, G):
    """m = 64, n = 4096, G in {256, 257, 1024} with ng in {1, 10, G, G + 5}: the c += 256 strides of mg_stats_kernel's LDS setup run once
    with nothing left over, once with one cluster left for a second trip, and four times up to MG_MAXG; rr = min(ng, G).  A stride that
    stopped at 256 would leave cluster 257's rank sum uninitialised.  With G = 256 the last cluster is ONE cell, and gene 5 is highest in
    that cell alone: its best cluster has n1 = 1, auc 1."""
    name = "many%d" % G
    X, label, G = _case(name)
    n = X.shape[1]
    for ng in (1, 10, G, G + 5):
        tab, info = _ref(name, 1e-4, ng)
        d = _dense(sa, X, label, G, 1e-4, ng)
        _check(d, tab, info, n, ng, "%s ng = %d" % (name, ng))
        if ng in (1, G + 5):
            _check_oracle(oracle, d, X, label, G, 1e-4, ng, np.arange(64), info, tab, name)
    assert np.array_equal(_ref(name, 1e-4, G)[0], _ref(name, 1e-4, G + 5)[0])
    s = _csc_whole(sa, X, label, G, 1e-4, G + 5)
    _check(s, tab, info, n, G + 5, name + " csc")
    _same_but_fc(d, s, name + " dense against csc")
    _same_but_fc(d, _dense(sa, X, label, G, 1e-4, G + 5), name + " twice")
    if G == 256:
        assert info["csize"][255] == 1 and d[5, 1] == 256.0 and d[5, 0] == 1.0


def test_cluster_count_refusals_time_no_kernel(sa):
    """G = 1025 and G = 1 are refused with the existing message before any kernel is timed"""
    from sharp_amd._lib import f64, i32

    L = sa.lib()
    X = np.asfortranarray(np.arange(12.0).reshape(3, 4))
    out = np.zeros((3, 5))
    L.sharp_profile_enable(1)
    L.sharp_profile_reset()
    try:
        for G, lab in ((1025, np.array([1, 2, 3, 1025], np.int32)), (1, np.ones(4, np.int32))):
            assert L.sharp_marker_genes(f64(X), 3, 4, 3, i32(lab), G, 1e-4, 1, f64(out)) != 0
            assert "between 2 and 1024 clusters are supported" in _err(sa)
        with pytest.raises(sa.SharpError, match="between 2 and 1024 clusters"):
            sa.get_marker_genes(np.arange(12.0).reshape(3, 4), {"pred_clusters": np.ones(4, np.int64)})
        ms, cnt = C.c_double(), C.c_longlong()
        for stage in STAGES:
            L.sharp_profile_get(stage, C.byref(ms), C.byref(cnt))
            assert cnt.value == 0, stage
    finally:
        L.sharp_profile_enable(0)


# ---- rank arithmetic ---------------------------------------------------------------------------------------------------------------------

def test_rank_arithmetic_edges(sa, oracle):
    """m = 40 planted genes (tests/_markers_ref.case_rank_arithmetic; premises asserted in tests/test_markers_cpu.py), n = 2000, G = 4
    clusters of 500, theta = 1e-3, ng in {1, 4}, dense and csc.  Able to fail: negative tie groups and three signs in one gene go through
    `shift` and `nneg` (a zero-group rank without 2 nneg moves every cluster's mean rank); t0 == 0 through the tie term's t0^3 - t0;
    sparsity == theta must give exactly (0, 0, 1, theta, 0), which `dp >= theta` would not; equal mean ranks and equal AUROCs must
    resolve to the first, which `>=` in either comparison would not; the all-tied gene's p is NaN on both sides; the one-cluster gene's
    FC is +inf; and the csc form carries -0.0 as STORED entries of gene 10, which must count as zeros exactly as the dense form's do."""
    X, label, G, idx = _case("rank_arithmetic")
    extra = np.signbit(X) & (X == 0)
    assert extra[idx["minus_zero"]].sum() > 600
    d = _full_case(sa, oracle, "rank_arithmetic", R.RANK_THETA, (1, 4), np.arange(40), extra=extra)
    assert d[idx["at_theta"]].tolist() == [0.0, 0.0, 1.0, R.RANK_THETA, 0.0]
    assert d[idx["equal_mean_rank"], 1] == 2.0 and d[idx["equal_auroc"], 1] == 3.0
    assert np.isnan(d[idx["all_tied"], 2]) and d[idx["all_tied"], 0] == 0.5 and d[idx["one_cluster_only"], 4] == np.inf
    res = sa.get_marker_genes(X, {"pred_clusters": np.asarray(label)}, theta=R.RANK_THETA, pvalue=2.0, auc=-1.0, FC=-1e300)
    assert res["gallinfo"]["gene"].tolist() == [g for g in range(40) if g not in (idx["at_theta"], idx["all_tied"])]


# ---- layouts and entries -----------------------------------------------------------------------------------------------------------------

def test_layouts_and_entries(sa, oracle):
    """m = 130, four blocks of 400 / 0 / 1 / 650 cells, G = 5.  sharp_marker_genes_dev on a tensor with ld = m + 6;
    sharp_marker_genes_blocks_dev with ld = m + 6, m, m + 2, m + 10 (the padding holds 99, which a wrong ld would read as counts);
    sharp_marker_genes_blocks_csc on slices of ONE larger dgCMatrix that starts with 7 foreign cells, so every colptr[b][0] != 0 and a
    missing rebase would read other cells' entries, with explicitly stored zeros and shuffled row indices within a cell; the empty block
    in both forms returns success (a dense block without cells is skipped: a grid of zero workgroups is no launch); a row index == m is
    refused; n m >= 2^40 is refused before anything is read."""
    import torch
    from sharp_amd._lib import f64, i32, i64

    X, label, G, sizes = _case("layouts")
    m, n = X.shape
    L = sa.lib()
    lab = np.ascontiguousarray(label, np.int32)
    cuts = np.cumsum([0] + sizes)
    for ng in (1, 5):
        tab, info = _ref("layouts", 1e-4, ng)
        # one resident block, ld = m + 6
        host = np.full((n, m + 6), 99.0, np.float32)
        host[:, :m] = X.T
        dX = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        out = np.full((m, 5), -7.0)
        rc = L.sharp_marker_genes_dev(dX.data_ptr(), m, n, m + 6, i32(lab), G, 1e-4, ng, f64(out))
        assert rc == 0, _err(sa)
        _check(out, tab, info, n, ng, "sharp_marker_genes_dev ld = m + 6")
        _check_oracle(oracle, out, X, label, G, 1e-4, ng, np.arange(m), info, tab, "layouts oracle")
        # a list of resident blocks, a different ld each; the empty one still needs an address
        lds = [m + 6, m, m + 2, m + 10]
        tens = []
        for b in range(4):
            h = np.full((max(sizes[b], 1), lds[b]), 99.0, np.float32)
            h[:sizes[b], :m] = X[:, cuts[b]:cuts[b + 1]].T
            tens.append(torch.from_numpy(h).cuda())
        torch.cuda.synchronize()
        ptrs = (C.c_void_p * 4)(*[t.data_ptr() for t in tens])
        outb = np.full((m, 5), -7.0)
        ncb, ldb = np.array(sizes, np.int64), np.array(lds, np.int64)
        rc = L.sharp_marker_genes_blocks_dev(ptrs, i64(ncb), i64(ldb), 4, m, i32(lab), G, 1e-4, ng, f64(outb))
        assert rc == 0, _err(sa)                                              # the block of zero cells is ordinary input
        _check(outb, tab, info, n, ng, "sharp_marker_genes_blocks_dev")
        _same_but_fc(out, outb, "one block against four")
        # slices of one larger CSC matrix: 7 foreign cells in front, stored zeros, shuffled rows within a cell
        rng = np.random.default_rng(5)
        front = np.full((m, 7), 5.0)
        big = np.concatenate([front, X], axis=1)
        extra = (big == 0) & (rng.random(big.shape) < 0.05)
        a = _stored(big, extra)
        indptr, indices, data = a.indptr.astype(np.int32), a.indices.astype(np.int32), a.data.astype(np.float64)
        assert np.count_nonzero(data == 0) > 1000
        for c in range(big.shape[1]):
            s, e = indptr[c], indptr[c + 1]
            o = rng.permutation(e - s)
            indices[s:e], data[s:e] = indices[s:e][o], data[s:e][o]
        slots = [(indptr[7 + cuts[b]: 7 + cuts[b + 1] + 1], indices, data, sizes[b]) for b in range(4)]
        assert all(s[0][0] != 0 for s in slots) and slots[1][0].size == 1
        outc = _csc(sa, slots, m, label, G, 1e-4, ng)
        _check(outc, tab, info, n, ng, "sharp_marker_genes_blocks_csc on slices")
        _same_but_fc(out, outc, "dense against csc slices")
    # refusals
    bad = indices.copy()
    bad[indptr[7 + 3]] = m
    rc = _csc(sa, [(s[0], bad, data, s[3]) for s in slots], m, label, G, 1e-4, 1, expect_ok=False)
    assert rc != 0 and "row index outside" in _err(sa)
    one = torch.zeros(1, dtype=torch.float32, device="cuda")
    huge = (1 << 40) // m + 1
    assert L.sharp_marker_genes_dev(one.data_ptr(), m, huge, m, i32(lab), G, 1e-4, 1, f64(out)) != 0
    assert "matrix too large" in _err(sa)
