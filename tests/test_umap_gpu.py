"""UMAP on the MI355X against the numpy specification (tests/_umap_ref.py).  Every stage is compared on the stage's own
input: the graph test feeds neighbour lists, the epoch test feeds the GPU's downloaded CSR and a given Y, so no stage inherits another's
rounding.  The full run is measured against the reference run's quality, recorded in §13."""
import ctypes as C

import numpy as np
import pytest

import _snn_ref
import _umap_ref as ref

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
# trustworthiness (sklearn, 15 neighbours) of the reference run on blobs(), seeds 10, 1, 2, 3, 4 (tests/test_umap_cpu.py)
REF_TRUST = (0.9607162566764462, 0.9599593169337245, 0.9605379673512375, 0.9608106522229745, 0.9600152561498533)


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


@pytest.fixture(scope="module")
def stages():
    from sharp_amd.umap import _epochs, _graph

    return _graph, _epochs


@pytest.fixture(scope="module")
def case():
    return ref.graph_case()


# ---- the graph ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [14, 64, 65, 255])
def test_graph_matches_the_reference(sa, stages, case, K):
    graph, _ = stages
    idx, d, rows = case
    idx, d = np.ascontiguousarray(idx[:, :K].astype(np.int32)), np.ascontiguousarray(d[:, :K])
    n = idx.shape[0]
    assert n == 1025 and n % 4 != 0
    rp, col, val, rho, sigma = graph(idx, d)
    rrho, rsigma, _, steps = ref.smooth_knn(d)
    # the special rows are what they are meant to be
    assert rrho[rows["dup_all"]] == 0 and (d[rows["dup_all"]] == 0).all()
    assert (d[rows["dup_some"]] == 0).sum() == 3 and rrho[rows["dup_some"]] > 0
    assert ref.row_sum_at(d[rows["far"]], rrho[rows["far"]], 1.0) < np.log2(K + 1) and rsigma[rows["far"]] > 1    # (the doubling branch)
    assert np.array_equal(rho, rrho)
    # every sigma satisfies the stopping rule as the reference evaluates it, or sits on its floor, or the bisection used all its steps
    target = np.log2(K + 1)
    total = d.sum()
    floor = np.where(rho > 0, d.sum(1) / (K + 1), total / (n * (K + 1))) * 1e-3
    stops = np.array([abs(ref.row_sum_at(d[i], rho[i], sigma[i]) - target) < 1e-5 for i in range(n)])
    on_floor = np.abs(sigma - floor) <= 1e-12 * floor
    assert (stops | on_floor | (steps == 64)).all()
    assert on_floor[rows["dup_all"]] and stops[rows["far"]]
    share = (np.abs(sigma - rsigma) <= 1e-12 * rsigma).mean()
    print(f"K = {K}: share of rows with the reference's sigma {share}")
    assert share >= 0.99
    _check_union(idx, d, rp, col, val, rho, sigma, f"K = {K}")


def _check_union(idx, d, rp, col, val, rho, sigma, label, one_sided=True, two_sided=True):
    """W on the stage's own rho and sigma against the reference's union: the pattern exactly, the values to the bound below;
    one_sided / two_sided: whether the lists hold pairs named in one direction only / in both"""
    n = idx.shape[0]
    # W on the stage's own rho and sigma: the reference's pattern exactly
    A = ref.weights(d, rho, sigma)
    wrp, wcol, x, y = ref.union_parts(idx, A, n)
    assert np.array_equal(rp, wrp) and np.array_equal(col, wcol)
    _, _, want = ref.fuzzy_union(idx, A, n)
    one, both = np.isnan(y) | np.isnan(x), ~np.isnan(x) & ~np.isnan(y)
    assert one.any() == one_sided and both.any() == two_sided
    assert np.array_equal(want[both], (x + y - x * y)[both]) and np.array_equal(want[one], np.where(np.isnan(y), x, y)[one])
    # Bound.  A weight is exp(-t), t = (d - rho) / sigma: the quotient carries one rounding (relative eps, so |t| eps absolute in the
    # exponent, |t| eps relative in the weight) and exp at most one ulp, on either side: 2 (1 + |t|) eps relative for a weight <= 1.
    # x + y - x y has partial derivatives in [0, 1] and three roundings of values <= 2: together below 4 eps (1 + t_ij + t_ji), absolute
    # (t = 0 for the absent direction and for a weight that is exactly 1).
    T = np.where(d - rho[:, None] > 0, (d - rho[:, None]) / sigma[:, None], 0.0)
    _, _, tx, ty = ref.union_parts(idx, T, n)
    tol = 4 * EPS * (1 + np.nan_to_num(tx) + np.nan_to_num(ty))
    err = np.abs(val - want)
    print(f"{label}: largest |W - reference| / bound {(err / tol).max()}")
    assert (err <= tol).all()
    # mirrored entries carry the same bits (x + y - x y is commutative), so they fire together
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    key = row * n + col
    mirror = np.searchsorted(key, col.astype(np.int64) * n + row)
    assert np.array_equal(val[mirror], val)


def _ring_lists(n, K):
    """row i names i + 1 .. i + K mod n, with distances that ascend along a row and differ between rows"""
    idx = _snn_ref.ring(n, K)
    d = np.sort(np.random.default_rng(n * 1000 + K).uniform(0.5, 2.0, size=(n, K)), axis=1)
    return idx, d


# The edges of the CSR builder behind the union (sort by row * n + col, merge equal keys, split the keys) that random lists do not pin down.
def test_graph_without_a_mutual_pair(sa, stages):
    """a directed ring, n = 40, K = 3: i names j and j names i never both (that needs a + b = 0 mod 40 with a, b in 1 .. 3), so no key
    appears twice and nothing is merged"""
    graph, _ = stages
    idx, d = _ring_lists(40, 3)
    rp, col, val, rho, sigma = graph(idx, d)
    assert col.size == 2 * 40 * 3 and np.array_equal(np.diff(rp), np.full(40, 6))
    _check_union(idx, d, rp, col, val, rho, sigma, "ring 40 x 3", two_sided=False)


def test_graph_with_every_pair_mutual(sa, stages):
    """the complete graph, n = K + 1 = 9: every key appears twice"""
    graph, _ = stages
    n = 9
    idx = _snn_ref.complete_lists(n)
    d = np.sort(np.random.default_rng(9).uniform(0.5, 2.0, size=(n, n - 1)), axis=1)
    rp, col, val, rho, sigma = graph(idx, d)
    assert col.size == n * (n - 1) and np.array_equal(col.reshape(n, n - 1), idx)
    _check_union(idx, d, rp, col, val, rho, sigma, "complete 9", one_sided=False)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_graph_where_the_key_width_changes(sa, stages, n):
    """n * n reaches 2^16 at n = 256, so the sort's end bit (the width of n * n) moves from 16 to 17; the largest key, the last row's
    last column (n - 1, n - 2), must come out last"""
    graph, _ = stages
    idx, d = _ring_lists(n, 5)
    assert (n * n).bit_length() == (16 if n == 255 else 17)
    rp, col, val, rho, sigma = graph(idx, d)
    assert rp[n] == col.size == 2 * n * 5 and rp[n - 1] < rp[n] and col[-1] == n - 2
    assert col[0] == 1 and rp[0] == 0 and rp[1] == 10                # (row 0: the columns 1 .. 5 and n - 5 .. n - 1)
    _check_union(idx, d, rp, col, val, rho, sigma, f"ring {n} x 5", two_sided=False)


# ---- one epoch ------------------------------------------------------------------------------------------------------------------------
def _hub_lists():
    """one centre plus 700 points on the unit sphere in 10-D, K = 64: the centre is among the 64 nearest of every one of them (with
    K = 14 it is among nobody's: 700 random points on that sphere have closer neighbours), so its row has degree 700"""
    rng = np.random.default_rng(3)
    P = rng.normal(size=(700, 10))
    P /= np.linalg.norm(P, axis=1)[:, None]
    return ref.knn_lists(np.vstack([np.zeros((1, 10)), P]), 64)


@pytest.fixture(scope="module")
def epoch_graphs(sa, stages, case):
    """the GPU's own CSR for the three inputs"""
    graph, _ = stages
    idx, d, _ = case
    out = {"n1025": graph(np.ascontiguousarray(idx[:, :14].astype(np.int32)), np.ascontiguousarray(d[:, :14]))[:3]}
    i40, d40 = ref.knn_lists(np.random.default_rng(2).normal(size=(40, 3)), 14)
    out["n40"] = graph(i40.astype(np.int32), d40)[:3]
    ih, dh = _hub_lists()
    out["hub"] = graph(ih.astype(np.int32), dh)[:3]
    assert np.diff(out["hub"][0])[0] == 700 > 640                    # the multi-pass row (64 lanes x 6 terms would hold 10 edges a pass)
    return out


@pytest.mark.parametrize("dims", [1, 2, 3])
@pytest.mark.parametrize("name", ["n1025", "n40", "hub"])
def test_one_epoch_matches_the_reference(sa, stages, epoch_graphs, name, dims):
    _, epochs = stages
    rp, col, val = epoch_graphs[name]
    n = rp.size - 1
    a, b = sa.umap_ab(1.0, 0.01)
    n_epochs = 10
    Y = np.random.default_rng(dims).uniform(0, 10, size=(n, dims))
    row = np.repeat(np.arange(n), np.diff(rp))
    e1 = int(np.argmax(val))                                         # an edge of rate 1: it fires in every epoch >= 1
    i1, j1 = int(row[e1]), int(col[e1])
    Y[j1] = Y[i1]                                                    # a coincident pair joined by that edge (D = 0)
    near = [int(k) for k in ref.draw(10, 7, np.full(5, e1), np.arange(5), n) if k not in (i1, j1)][0]
    Y[near] = Y[i1] + 0.02 / np.sqrt(dims)                           # a vertex that edge draws in epoch 7, 0.02 away (the clip)
    # a far pair joined by an edge of rate 1.  (With b < 1 the attraction never reaches the clip, near or far: |c_att| |y_i - y_j| stays
    # near 1 at most; the clip acts on the repulsion of the vertex 0.02 away.)
    e2 = [int(e) for e in np.nonzero(val == val.max())[0] if not {int(row[e]), int(col[e])} & {i1, j1, near}][0]
    i2, j2 = int(row[e2]), int(col[e2])
    Y[j2] = Y[i2] + 30.0 / np.sqrt(dims)
    assert (Y[j1] == Y[i1]).all() and abs(np.linalg.norm(Y[j2] - Y[i2]) - 30.0) < 1e-9
    clipped_any = 0
    selfdraw = 0
    for ep in (1, 7, n_epochs - 1):
        want, terms, clipped = ref.epoch(rp, col, val, Y, ep, n_epochs, a, b, seed=10, return_terms=True)
        got = epochs(rp, col, val, Y, n_epochs, ep, ep + 1, a, b, seed=10)
        alpha = 1.0 - ep / n_epochs
        # Bound.  A term is clip(c (y_i - y_k)) in [-4, 4] (the attraction twice that, counted once in `terms` and covered by the factor
        # below): c comes from two fp64 pow calls, a sum of <= 3 squares, a division and three products -- a few eps relative each,
        # well inside 32 eps -- so a term is off by at most 4 * 32 eps, and the row's sum, scaled by alpha, by terms * 4 * 32 eps * alpha.
        bound = terms * 4 * 32 * EPS * alpha
        err = np.abs(got - want).max(1)
        print(f"{name} dims {dims} ep {ep}: firing rows {(terms > 0).sum()}, largest err / bound "
              f"{(err[terms > 0] / bound[terms > 0]).max() if (terms > 0).any() else 0.0}")
        assert (err <= bound).all()
        assert np.array_equal(got[terms == 0], Y[terms == 0])        # a row without a firing edge stays where it is
        assert (terms > 0).any()
        clipped_any += clipped
        f = np.nonzero(ref.fires(ep, val / val.max()))[0]
        selfdraw += sum(int((ref.draw(10, ep, f, s, n) == row[f]).sum()) for s in range(5))
    assert clipped_any > 0                                           # the clip acted
    if name == "n40":
        assert selfdraw > 0                                          # self-draws k = i occurred
    if name == "hub":
        assert terms[0] >= 64 * 6                                    # (the centre's own 64 edges have rate 1)


def test_epoch_zero_moves_nothing(sa, stages, epoch_graphs):
    _, epochs = stages
    rp, col, val = epoch_graphs["n40"]
    Y = np.random.default_rng(0).uniform(0, 10, size=(40, 2))
    assert np.array_equal(epochs(rp, col, val, Y, 10, 0, 1, 1.9, 0.8), Y)


# ---- properties of the optimiser ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_resume_gives_the_bits_of_one_run(sa, stages, epoch_graphs, dims):
    _, epochs = stages
    rp, col, val = epoch_graphs["n1025"]
    Y = np.random.default_rng(10 + dims).uniform(0, 10, size=(rp.size - 1, dims))
    whole = epochs(rp, col, val, Y, 7, 0, 7, 1.9, 0.8, seed=4)
    part = epochs(rp, col, val, epochs(rp, col, val, Y, 7, 0, 3, 1.9, 0.8, seed=4), 7, 3, 7, 1.9, 0.8, seed=4)
    assert np.array_equal(whole, part) and not np.array_equal(whole, Y)
    assert not np.array_equal(whole, epochs(rp, col, val, Y, 7, 0, 7, 1.9, 0.8, seed=5))


@pytest.fixture(scope="module")
def blobs():
    return ref.blobs()


def test_two_calls_are_bitwise_equal_and_lists_fed_back_give_the_same_bits(sa, blobs):
    X, _ = blobs
    r1 = sa.umap(X, n_epochs=60, ret_nn=True)
    r2 = sa.umap(X, n_epochs=60)
    assert np.array_equal(r1["Y"], r2["Y"]) and np.isfinite(r1["Y"]).all()
    assert (r1["a"], r1["b"]) == sa.umap_ab(1.0, 0.01) and r1["n_epochs"] == 60
    ri, rd = sa.knn(X, 14)
    assert np.array_equal(r1["nn"]["index"], ri) and np.array_equal(r1["nn"]["distance"], rd)
    Y0 = np.random.default_rng(1).normal(size=(X.shape[0], 2))
    direct = sa.umap(X, n_epochs=60, init=Y0)
    fed = sa.umap_neighbors(*sa.knn(X, 14), n_epochs=60, init=Y0)
    assert np.array_equal(direct["Y"], fed["Y"])
    fed2 = sa.umap_neighbors(*sa.knn(X, 14, squared=True), squared=True, n_epochs=60, init=Y0)
    assert np.array_equal(direct["Y"], fed2["Y"])
    assert not np.array_equal(direct["Y"], r1["Y"])
    ra = sa.umap(X, n_epochs=20, init="random", seed=3)
    rb = sa.umap(X, n_epochs=20, init="random", seed=3)
    rc = sa.umap(X, n_epochs=20, init="random", seed=4)
    assert np.array_equal(ra["Y"], rb["Y"]) and not np.array_equal(ra["Y"], rc["Y"])


def test_start_is_the_scaled_pca_and_the_library_refuses_bad_input(sa, blobs):
    X, _ = blobs
    for dims in (1, 2, 3):
        y0 = sa.umap(X, n_components=dims, n_epochs=0)["Y"]
        assert np.allclose(y0.min(0), 0) and np.allclose(y0.max(0), 10)
        want = ref.scale_start(ref.pca_start(X, dims))
        assert np.abs(y0 - want).max() < 1e-8
    yr = sa.umap(X, n_epochs=0, init="random")["Y"]
    assert np.allclose(yr.min(0), 0) and np.allclose(yr.max(0), 10)
    yc = sa.umap(X, n_epochs=0, init=np.column_stack([np.arange(1500.0), np.full(1500, 3.0)]))["Y"]
    assert np.array_equal(yc[:, 1], np.zeros(1500)) and yc[:, 0].max() == 10          # a constant coordinate becomes 0
    bad = X.copy()
    bad[17, 3] = np.nan
    with pytest.raises(sa.SharpError, match=r"NA / NaN / Inf \(row 18, column 4\)"):
        sa.umap(bad)
    idx, d = sa.knn(X, 14)
    wrong = idx.copy()
    wrong[5, 2] = 1500
    with pytest.raises(sa.SharpError, match=r"^umap_neighbors: a neighbour index outside \[0, n\) \(row 5,"):
        sa.umap_neighbors(wrong, d)
    with pytest.raises(sa.SharpError, match=r"^umap: "):
        sa.umap(bad)
    assert np.isfinite(sa.umap(X, n_epochs=5, pca=5)["Y"]).all()     # (the library is usable after a refusal; the pca argument)


# ---- the full run ---------------------------------------------------------------------------------------------------------------------
def test_full_run_separates_the_blobs(sa, blobs):
    X, lab = blobs
    out = sa.umap(X)
    Y = out["Y"]
    assert out["n_epochs"] == 500 and Y.shape == (1500, 2) and np.isfinite(Y).all()
    purity = ref.knn_purity(Y, lab, 15)
    print("15-NN label purity of the GPU map:", purity)
    assert purity >= 1.0                                             # the reference run's, minus nothing
    manifold = pytest.importorskip("sklearn.manifold")
    t = manifold.trustworthiness(X, Y, n_neighbors=15)
    floor = min(REF_TRUST) - 3 * (max(REF_TRUST) - min(REF_TRUST))
    print(f"trustworthiness of the GPU map {t}, the reference's five-seed minimum minus three spreads {floor}")
    assert t >= floor


def test_visualization_sharp_method_umap(sa, oracle):
    from sharp_amd.api import _vis_input

    X = oracle.synth_fill(20261003, 1500, 0, 1200, 4, 200)
    res = sa.SHARP(X, rN_seed=2103, ensize_K=3)
    v = sa.visualization_SHARP(res, method="umap", plot=False, n_epochs=50, return_neighbors=True)
    assert v["Y"].shape == (1200, 2) and np.isfinite(v["Y"]).all() and v["n_epochs"] == 50
    nb = v["neighbors"]
    assert nb["index"].shape == (1200, 14) and nb["squared"] is False and nb["n"] == 1200 and nb["w"] == 2
    again = sa.visualization_SHARP(res, method="umap", plot=False, n_epochs=50, neighbors=nb)
    assert np.array_equal(again["Y"], v["Y"]) and "neighbors" not in again
    # the lists do not depend on the method: a t-SNE call's lists serve the UMAP map (their first 14 columns) with the same bits
    t = sa.visualization_SHARP(res, plot=False, max_iter=20, return_neighbors=True)
    assert np.array_equal(t["neighbors"]["index"][:, :14], nb["index"])
    via = sa.visualization_SHARP(res, method="umap", plot=False, n_epochs=50, neighbors=t["neighbors"])
    assert np.array_equal(via["Y"], v["Y"])
    # given lists and a given start: x1 is neither built nor prepared (a result without x0 / viE columns of use would do)
    rnd = sa.visualization_SHARP(res, method="umap", plot=False, n_epochs=5, neighbors=nb, init="random")
    assert np.array_equal(rnd["Y"], sa.umap_neighbors(nb["index"], nb["distance"], n_epochs=5, init="random")["Y"])
    with pytest.raises(sa.SharpError, match="needs 99 neighbours"):
        sa.visualization_SHARP(res, method="umap", plot=False, n_neighbors=100, neighbors=t["neighbors"])
    # the default is still Rtsne's map
    x1 = _vis_input(res, 2)
    want = sa.Rtsne(x1, check_duplicates=False, pca=x1.shape[1] > 50, max_iter=20, seed=10)["Y"]
    assert np.array_equal(t["Y"], want)
    assert np.array_equal(sa.visualization_SHARP(res, plot=False, max_iter=20)["Y"], want)
    assert np.array_equal(sa.visualization_SHARP(res, plot=False, max_iter=20, method="tsne")["Y"], want)


# ---- the .C() twins -------------------------------------------------------------------------------------------------------------------
def test_dotc_twins(sa, blobs):
    """the .C() convention (tests/test_dotc_gpu.py): same outputs as the C entries, status set on a refusal"""
    L = sa.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    I = lambda v: np.array([v], np.int32)                            # noqa: E731
    D = lambda v: np.array([v], np.float64)                          # noqa: E731
    X = np.ascontiguousarray(blobs[0][:600])
    n, K = 600, 14
    Y, st, ab = np.zeros((n, 2)), I(-1), np.zeros(2)
    nn_i, nn_d = np.zeros((n, K), np.int32), np.zeros((n, K))
    opt = [I(2), I(40), D(1.0), D(0.01), D(1.0), ab, I(5), D(1.0)]
    L.sharp_C_umap(*[P(v) for v in [X, D(n), I(10), I(15)] + opt + [I(0), np.zeros(1), I(0), I(1), D(10.0), Y, I(1), nn_i, nn_d, st]])
    want = sa.umap(X, n_epochs=40, ret_nn=True)
    assert st[0] == 0 and np.array_equal(Y, want["Y"]) and (ab[0], ab[1]) == (want["a"], want["b"])
    assert np.array_equal(nn_i, want["nn"]["index"]) and np.array_equal(nn_d, want["nn"]["distance"])
    Y0 = np.random.default_rng(5).normal(size=(n, 2))
    Y[:], st[0] = 0, -1
    ab2 = np.array([1.5, 0.9])
    opt[5] = ab2
    L.sharp_C_umap_neighbors(*[P(v) for v in [nn_i, nn_d, D(n), I(K), I(0)] + opt + [I(2), Y0, D(10.0), Y, st]])
    want = sa.umap_neighbors(nn_i, nn_d, n_epochs=40, init=Y0, a=1.5, b=0.9)
    assert st[0] == 0 and np.array_equal(Y, want["Y"]) and (ab2[0], ab2[1]) == (1.5, 0.9)
    # want_nn = 0 leaves the buffers alone; init = 1 draws the start from the seed
    keep = nn_i.copy()
    L.sharp_C_umap(*[P(v) for v in [X, D(n), I(10), I(15)] + opt + [I(1), np.zeros(1), I(0), I(1), D(3.0), Y, I(0), nn_i, nn_d, st]])
    assert st[0] == 0 and np.array_equal(nn_i, keep)
    assert np.array_equal(Y, sa.umap(X, n_epochs=40, init="random", seed=3, a=1.5, b=0.9)["Y"])
    # refusals: the status and the message
    buf = C.create_string_buffer(b" " * 255)
    msg, ln = (C.c_char_p * 1)(C.addressof(buf)), (C.c_int * 1)(256)
    bad = nn_i.copy()
    bad[17, 4] = n
    L.sharp_C_umap_neighbors(*[P(v) for v in [bad, nn_d, D(n), I(K), I(0)] + opt + [I(2), Y0, D(10.0), Y, st]])
    L.sharp_C_last_error(msg, ln)
    assert st[0] == 2 and b"outside [0, n) (row 17," in buf.value
    L.sharp_C_umap(*[P(v) for v in [X, D(n), I(10), I(600)] + opt + [I(1), np.zeros(1), I(0), I(1), D(3.0), Y, I(0), nn_i, nn_d, st]])
    assert st[0] == 2
