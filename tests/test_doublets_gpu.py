"""scrublet() and its stages on the GPU against tests/_doublets_ref.py: the merge of two sorted sparse columns bit for bit
against scipy at the shapes where it can go wrong, the doublets' PCA scores bit for bit against expression_pca_transform of the
host-built blocks, the neighbour counts, the whole call's invariances and the quality floors of the numpy reference."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import _doublets_ref as R
import _expr_pca_ref as ref
from sharp_amd import doublets  # noqa: F401  (without the feature every test here fails at import)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


def host_doublets(blocks, parents):
    X = ref.concat(blocks)
    D = (X[:, parents[:, 0]] + X[:, parents[:, 1]]).tocsc()
    D.sort_indices()
    return D


def synth_raw(sa, blocks, parents, slab, cap, sentinel=-7):
    """sharp_doublet_synth_csc into outputs pre-filled with a sentinel: (status, colptr, rowidx, val, cell_sum)"""
    from sharp_amd import doublets
    from sharp_amd._lib import f64, i32, i64

    bl, m, n = doublets._counts(blocks, "simulate_doublets")
    args, keep = doublets._pointers(bl)
    ns = parents.shape[0]
    cp, ri, vx, cs = np.full(ns + 1, sentinel, np.int64), np.full(cap + 16, sentinel, np.int32), np.full(cap + 16, float(sentinel)), np.zeros(ns)
    st = sa.lib().sharp_doublet_synth_csc(*args, m, i64(parents), ns, slab, cap, i64(cp), i32(ri), f64(vx), f64(cs))
    del keep
    return st, cp, ri, vx, cs


# ---- synthesis --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand():
    blocks, par = R.hand_cells()
    return blocks, par, host_doublets(blocks, par)


@pytest.mark.parametrize("slab", [0, 7, 1])
def test_synthesis_bits(sa, hand, slab):
    blocks, par, want = hand
    cap = int(want.nnz)                                                       # exactly what the doublets need
    st, cp, ri, vx, cs = synth_raw(sa, blocks, par, slab, cap)
    assert st == 0, sa.lib().sharp_last_error()
    assert np.array_equal(cp, want.indptr) and (np.diff(cp) >= 0).all()
    assert np.array_equal(ri[:cap], want.indices) and vx[:cap].tobytes() == want.data.tobytes()
    assert (ri[cap:] == -7).all() and (vx[cap:] == -7.0).all()                # nothing behind colptr[n_sim] was written
    for s in range(par.shape[0]):
        g = ri[cp[s]:cp[s + 1]]
        assert (np.diff(g) > 0).all(), s                                      # strictly ascending: no gene twice
    assert np.array_equal(cs, np.asarray(want.sum(0)).ravel())
    D, L = R.synth(blocks, par)                                               # and the reference's own merge
    assert np.array_equal(cp, D.indptr) and np.array_equal(ri[:cap], D.indices) and np.array_equal(cs, L)


def test_synthesis_wrapper_and_capacity(sa, hand):
    blocks, par, want = hand
    got = sa.simulate_doublets(blocks, parents=par)
    assert (got["counts"] != want).nnz == 0 and np.array_equal(got["counts"].indices, want.indices) and np.array_equal(got["parents"], par)
    sim = sa.simulate_doublets(blocks, n_sim=90, seed=4, max_doublets_per_slab=11)
    assert np.array_equal(sim["parents"], R.pairs(40, 90, 4))
    assert (sim["counts"] != host_doublets(blocks, sim["parents"])).nnz == 0
    with pytest.raises(sa.SharpError, match="simulate_doublets: the doublets hold more stored entries than the capacity of rowidx / val"):
        sa.simulate_doublets(blocks, parents=par, capacity=int(want.nnz) - 1)
    with pytest.raises(sa.SharpError, match=r"simulate_doublets: a parent outside \[0, n\) \(doublet 1, counted from 0\)"):
        sa.simulate_doublets(blocks, parents=np.array([[0, 1], [2, 40]]))


# ---- projection -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted_blocks():
    return ref.ragged(ref.planted(600, 400, 4)[0], [0, 250, 251])


@pytest.mark.parametrize("subset", [True, False])
def test_projection_bits(sa, planted_blocks, subset):
    from sharp_amd import doublets

    blocks = planted_blocks
    G = np.sort(np.random.default_rng(3).choice(400, 120, replace=False)) if subset else None
    fit = sa.expression_pca(blocks, 8, oversample=4, n_iter=3, scale=True, seed=7, genes=G)
    par = np.vstack([R.pairs(600, 300, 5), [[0, 0], [599, 0], [250, 251], [17, 17]]])
    D = host_doublets(blocks, par)
    assert (D.data == np.floor(D.data)).all()
    want = sa.expression_pca_transform(ref.ragged(D, [100, 101]), fit)
    for slab in (0, 37):
        got = doublets._project(blocks, par, fit, slab)
        assert got.tobytes() == want.tobytes(), slab
    assert np.abs(want).max() > 1.0


# ---- neighbour counts -------------------------------------------------------------------------------------------------------------------
def test_neighbor_counts(sa):
    from sharp_amd import doublets

    rng = np.random.default_rng(11)
    n, ns, K = 300, 400, 70                                                   # K passes a wave's 64 lanes
    Z = np.vstack([rng.normal(size=(n - 100, 5)), rng.normal(size=(100, 5)) + 4.0,      # observed: alone, and among simulated
                   rng.normal(size=(200, 5)) + 4.0, rng.normal(size=(ns - 200, 5)) + 40.0])
    idx, _ = sa.knn(Z, K)
    got = doublets._neighbor_counts(idx, n)
    want = R.neighbor_counts(idx, n)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert (want == 0).any() and (want == K).any() and ((want > 0) & (want < K)).any()
    assert np.array_equal(doublets._neighbor_counts(idx[:, :1], n), R.neighbor_counts(idx[:, :1], n))
    assert np.array_equal(doublets._neighbor_counts(idx, 0), np.full(n + ns, K)) and not doublets._neighbor_counts(idx, n + ns).any()


# ---- the whole call ---------------------------------------------------------------------------------------------------------------------
KEYS = ("doublet_scores", "doublet_scores_sim", "neighbor_counts", "parents", "genes", "predicted_doublets")
SCALARS = ("threshold", "threshold_found", "detected_doublet_rate", "detectable_doublet_fraction", "overall_doublet_rate", "n_neighbors", "k_adj",
           "n_sim")


def same(a, b):
    for key in KEYS:
        assert (a[key] is None and b[key] is None) or a[key].tobytes() == b[key].tobytes(), key
    for key in SCALARS:
        assert a[key] == b[key], key


@pytest.fixture(scope="module")
def whole(sa):
    X = ref.planted(400, 400, 4)[0]
    return X, sa.scrublet(X, n_prin_comps=10, n_top_genes=150, ret_sim=True)


def test_whole_call_invariances(sa, whole):
    X, r = whole
    n = 400
    assert (r["n_sim"], r["n_neighbors"], r["k_adj"]) == R.plan(n) == (800, 10, 30)
    assert np.array_equal(r["parents"], R.pairs(n, 800, 0))
    same(r, sa.scrublet(X, n_prin_comps=10, n_top_genes=150))
    same(r, sa.scrublet(ref.ragged(X, [130, 131]), n_prin_comps=10, n_top_genes=150, max_doublets_per_slab=97))
    hv = sa.highly_variable_genes(X, 150)
    assert np.array_equal(r["genes"], hv["genes"])
    pc = sa.expression_pca(X, 10, scale=True, genes=hv["genes"])
    same(r, sa.scrublet(X, pca=pc))
    same(r, sa.scrublet(X, genes=hv["genes"], n_prin_comps=10))
    # the stages behind the result
    D = host_doublets([X], r["parents"])
    assert r["sim_pca"].tobytes() == sa.expression_pca_transform(D, pc).tobytes()
    Z = np.vstack([pc["scores"], r["sim_pca"]])
    idx, _ = sa.knn(Z, 30)
    assert np.array_equal(r["neighbor_counts"], R.neighbor_counts(idx, n))
    table = R.score_table(30, 2.0, 0.1)
    assert r["doublet_scores"].tobytes() == table[r["neighbor_counts"][:n]].tobytes()
    assert r["doublet_scores_sim"].tobytes() == table[r["neighbor_counts"][n:]].tobytes()
    t = R.threshold(r["doublet_scores"], r["doublet_scores_sim"])
    assert t["threshold"] == r["threshold"] and t["threshold_found"] == r["threshold_found"]
    if t["threshold_found"]:
        assert np.array_equal(t["predicted_doublets"], r["predicted_doublets"])
        assert (t["detected_doublet_rate"], t["detectable_doublet_fraction"], t["overall_doublet_rate"]) == (
            r["detected_doublet_rate"], r["detectable_doublet_fraction"], r["overall_doublet_rate"])
    g = sa.scrublet(X, pca=pc, threshold=0.25)
    assert g["threshold"] == 0.25 and not g["threshold_found"] and np.array_equal(g["predicted_doublets"], r["doublet_scores"] > 0.25)


def test_whole_call_descent(sa, whole):
    X, r = whole
    pc = sa.expression_pca(X, 10, scale=True, genes=r["genes"])
    args = {"n_projections": 4, "seed": 3}
    d = sa.scrublet(X, pca=pc, nn_method="descent", nn_args=args)
    same(d, sa.scrublet(X, pca=pc, nn_method="descent", nn_args=args))
    idx, _ = sa.knn_descent(np.vstack([pc["scores"], r["sim_pca"]]), 30, **args)
    assert np.array_equal(d["neighbor_counts"], R.neighbor_counts(idx, 400))
    with pytest.raises(sa.SharpError, match="scrublet: nn_args belong to nn_method"):
        sa.scrublet(X, pca=pc, nn_args=args)


def test_no_threshold_warns(sa):
    """twenty copies of one cell: every doublet is that cell again, every row's neighbours are observed, the simulated scores are one value"""
    rng = np.random.default_rng(2)
    col = sp.csc_matrix(rng.integers(0, 5, size=(30, 1)).astype(np.float64))
    X = sp.hstack([col] * 20, format="csc")
    fit = {"loadings": rng.normal(size=(30, 2)), "center": np.zeros(30), "scale": np.ones(30), "normalize_total": 1e4, "log1p": True, "genes": None}
    fit["scores"] = sa.expression_pca_transform(X, fit)
    with pytest.warns(RuntimeWarning, match="scrublet: no threshold found: the histogram of the simulated doublets' scores never shows two modes"):
        r = sa.scrublet(X, pca=fit)
    assert r["threshold"] is None and not r["threshold_found"] and r["predicted_doublets"] is None and r["overall_doublet_rate"] is None
    assert not r["neighbor_counts"].any() and np.unique(r["doublet_scores_sim"]).size == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        g = sa.scrublet(X, pca=fit, threshold=0.5)
    assert g["threshold"] == 0.5 and not g["predicted_doublets"].any()


# ---- quality ----------------------------------------------------------------------------------------------------------------------------
def test_quality_meets_the_reference_floor(sa):
    """The planted input with 8 % planted doublets.  The floors are the numpy reference's worst value over five seeds less its
    seed-to-seed spread (tests/test_doublets_cpu.py; measured 0.99992 for the AUROC and 0.942 for the share above the threshold)."""
    X, is_d = R.quality_input()
    q = R.quality_reference()
    r = sa.scrublet(X, n_top_genes=R.TOP_QUALITY)
    au = R.auroc(r["doublet_scores"], is_d)
    share = float(r["predicted_doublets"][is_d].mean()) if r["threshold_found"] else 0.0
    print("AUROC", au, "floor", q["auroc_floor"], "share", share, "floor", q["share_floor"], "threshold", r["threshold"])
    assert r["threshold_found"]
    assert au >= q["auroc_floor"]
    assert share >= q["share_floor"]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_library(sa, planted_blocks):
    """what the Python layer refuses first (tests/test_doublets_cpu.py) the library refuses too, by the same names"""
    import ctypes as C

    from sharp_amd import doublets
    from sharp_amd._lib import f64, i32, i64

    X = sp.csc_matrix(np.random.default_rng(0).integers(0, 4, size=(30, 12)).astype(np.float64))

    def call(X, ratio=2.0, rho=0.1, nn=0, seed=0):
        bl, m = [X.tocsc()], X.shape[0]                                       # (past the Python layer's own checks)
        args, keep = doublets._pointers(bl)
        big = 64
        out = (f64(np.zeros(big)), f64(np.zeros(big)), i32(np.zeros(big, np.int32)), C.byref(C.c_double()), C.byref(C.c_int()), f64(np.zeros(3)),
               C.byref(C.c_int()), C.byref(C.c_int()), i64(np.zeros(2 * big, np.int64)), i32(np.zeros(big, np.int32)), C.byref(C.c_int()),
               i32(np.zeros(2 * big, np.int32)), None)
        st = sa.lib().sharp_scrublet_csc(*args, m, ratio, rho, nn, 3, 10, None, 0, None, None, None, None, 1e4, 1, 1, float("nan"), 0, None, seed, 0,
                                         *out)
        del keep
        return st, sa.lib().sharp_last_error().decode()

    bad = X.copy()
    bad.data[5] = -1.0
    cases = [((bad,), {}, "scrublet: a negative value where counts are expected (cell"),
             ((X[:, :1],), {}, "scrublet: need at least 2 cells in all"),
             ((X,), {"ratio": 0.01}, "scrublet: sim_doublet_ratio gives fewer than 1 simulated doublet"),
             ((X,), {"rho": 1.0}, "scrublet: expected_doublet_rate must lie in (0, 1)"),
             ((X,), {"seed": 2 ** 53}, "scrublet: seed must be a whole number in [0, 2^53)"),
             ((X,), {"nn": 30}, "scrublet: n_neighbors = 30 gives k_adj = 90 neighbours per row; there are only n + n_sim - 1 = 35 other rows")]
    bad2 = X.copy()
    bad2.data[7] = np.nan
    cases.append(((bad2,), {}, "scrublet: a value that is NaN or infinite (cell"))
    for a, kw, msg in cases:
        st, err = call(*a, **kw)
        assert st != 0 and msg in err, (msg, err)
