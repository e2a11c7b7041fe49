"""umap_transform on the MI355X against the numpy specification (tests/_umap_transform_ref.py).  Every stage is compared
on the stage's own input: the weights test feeds lists, the epoch test feeds lists, weights and a given Y, so no stage inherits
another's rounding.  The invariant (a row's result does not depend on the rows beside it, the launch split or the block it travels in) is
checked bit for bit; the full run is measured against the reference run's quality, recorded in §14."""
import ctypes as C

import numpy as np
import pytest

import _umap_ref as ref
import _umap_transform_ref as tr

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
AB = (1.8956058664239412, 0.8006378441176886)       # any positive pair serves the stage tests (about the default curve's)


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


@pytest.fixture(scope="module")
def stages():
    from sharp_amd.umap import _knn_cross, _transform_epochs, _transform_weights

    return _knn_cross, _transform_weights, _transform_epochs


@pytest.fixture(scope="module")
def cases():
    """{d: (X_ref, Xq, the reference's 255 nearest of every query: idx, Euclidean distances)}, computed once: the first K columns of a
    (distance, index)-sorted list are the K-NN list"""
    out = {}
    for d in tr.DS:
        X, lab = tr.reference_rows(d)
        Q, _ = tr.queries(X, lab)
        assert X.shape == (1025, d) and Q.shape == (333, d) and 1025 % 64 and 333 % 16
        out[d] = (X, Q) + tr.cross_knn(X, Q, 255)
    return out


def _map(n, dims, seed=4):
    return np.random.default_rng(seed).uniform(-10, 10, size=(n, dims))


@pytest.fixture(scope="module")
def models(sa, cases):
    """a model per input width (2-D maps), and for d = 10 one per map dimension; n_neighbors 15, the fit's epochs 90 (so E = 30)"""
    out = {d: sa.UmapModel(cases[d][0], _map(1025, 2), 15, AB[0], AB[1], 90) for d in tr.DS}
    for dims in (1, 3):
        out[10, dims] = sa.UmapModel(cases[10][0], _map(1025, dims), 15, AB[0], AB[1], 90)
    out[10, 2] = out[10]
    yield out
    for m in out.values():
        m.close()


# ---- the cross k-NN -------------------------------------------------------------------------------------------------------------------
def _check_lists(X, Q, gi, gd, ri, d):
    """indices identical to the reference's; squared distances within 4 eps d max term of the direct sum"""
    assert gi.dtype == np.int32 and np.array_equal(gi, ri)
    t = (Q[:, None, :] - X[ri]) ** 2                                  # the terms of the direct sum, nq x K x d
    err = np.abs(gd * gd - t.sum(2))
    bound = 4 * EPS * d * t.max(2)
    print(f"largest |d^2 - reference| / bound {(err[bound > 0] / bound[bound > 0]).max()}")
    assert (err <= bound).all()
    assert (np.diff(gd, axis=1) >= 0).all()


@pytest.mark.parametrize("d,K", [(d, K) for d in (3, 10, 50) for K in tr.KS] + [(70, 15)])
def test_cross_knn_matches_the_reference(sa, stages, cases, models, d, K):
    """d = 3, 10: no multiple of 4; 50: the register path's last, partial k-step; 70: the LDS panel.  333 rows are no multiple of 16,
    1 025 reference rows no multiple of 64.  tests/test_umap_transform_cpu.py holds the premise (every row's gap) of the exact comparison."""
    knn_cross = stages[0]
    X, Q, ri, _ = cases[d]
    gi, gd = sa.knn_query(models[d], Q, K)
    _check_lists(X, Q, gi, gd, ri[:, :K], d)
    # several launches and a last partial one (333 = 6 x 48 + 45): bit for bit the same lists
    si, sd = knn_cross(models[d], Q, K, max_rows_per_launch=48)
    assert np.array_equal(si, gi) and np.array_equal(sd, gd)


def test_cross_knn_exact_copy_and_ties(sa, cases):
    """a query copied from a reference row that has a duplicate: distance 0 twice, the lower index first"""
    X, Q, _, _ = cases[10]
    X, Q = X.copy(), Q.copy()
    X[700] = X[123]
    Q[5] = X[123]
    Q[6] = X[700]
    gi, gd = sa.knn_query(X, Q, 15)
    assert list(gi[5, :2]) == [123, 700] and list(gd[5, :2]) == [0.0, 0.0] and gd[5, 2] > 0
    assert list(gi[6, :2]) == [123, 700] and list(gd[6, :2]) == [0.0, 0.0]
    ri, _ = tr.cross_knn(X, Q, 15)
    _check_lists(X, Q, gi, gd, ri, 10)


def test_cross_knn_far_from_the_origin(sa, cases):
    """the whole input translated by 1e4: centring by the model's mean keeps the lists (the GEMM form on the raw values would err by
    eps * 1e8 * d, far above the gaps)"""
    X, Q, ri, _ = cases[10]
    Xt, Qt = X + 1e4, Q + 1e4
    gi, gd = sa.knn_query(Xt, Qt, 15)
    _check_lists(Xt, Qt, gi, gd, tr.cross_knn(Xt, Qt, 15)[0], 10)
    assert np.array_equal(gi, ri[:, :15])


# ---- weights and start ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,dims", [(K, 2) for K in tr.KS] + [(15, 1), (15, 3)])
def test_weights_and_start_match_the_reference(sa, stages, cases, models, K, dims):
    weights = stages[1]
    m = models[10, dims]
    Y_ref = _map(1025, dims)
    idx = np.ascontiguousarray(cases[10][2][:, :K].astype(np.int32))
    d = np.ascontiguousarray(cases[10][3][:, :K])
    d[5] = 50.0 * np.arange(K)                                       # the doubling branch
    d[6] = 0.0                                                       # K zero distances
    sigma, w, Y0 = weights(m, idx, d)
    rsigma, _, _, steps = tr.smooth(d)
    target = np.log2(K)
    floor = 1e-3 * d.sum(1) / K
    stops = np.array([abs(tr.row_sum_at(d[q], sigma[q]) - target) < 1e-5 for q in range(333)])
    on_floor = np.abs(sigma - floor) <= 1e-12 * floor
    assert (stops | on_floor | (steps == 64)).all()
    assert tr.row_sum_at(d[5], 1.0) < target and sigma[5] > 1 and stops[5]
    # K zero distances are handled, not refused: the sum is K at every sigma, so the bisection halves 64 times and the floor is 0:
    # sigma = 2^-64, every weight exp(-0) = 1, the start the plain mean of the K positions
    assert sigma[6] == 2.0 ** -64 and (w[6] == 1).all()
    share = (np.abs(sigma - rsigma) <= 1e-12 * rsigma).mean()
    print(f"K = {K}: share of rows with the reference's sigma {share}")
    assert share >= 0.99
    # a weight is exp(-t), t = d / sigma: one rounding in the quotient (t eps in the exponent) and one ulp of exp on either side
    want = tr.weights(d, sigma)
    tol = 4 * EPS * (1 + d / sigma[:, None])
    assert (np.abs(w - want) <= tol).all()
    # the start on the stage's own weights: K products and sums of values up to max |Y_ref|, one division
    err = np.abs(Y0 - tr.start(idx.astype(np.int64), w, Y_ref))
    print(f"K = {K}, dims {dims}: largest start error / bound {err.max() / (4 * EPS * K * np.abs(Y_ref).max())}")
    assert (err <= 4 * EPS * K * np.abs(Y_ref).max()).all()


def test_start_of_a_row_whose_weight_underflows(sa, stages, cases, models):
    """K = 1 and a distance of 800: exp(-800) = 0 meets the target log2 1 = 0 at once, sigma = max(1, 0.8), the only weight is 0 and the
    row starts at its neighbour; a zero distance gives sigma = 2^-64 and weight 1 (tests/test_umap_transform_cpu.py has the reference's)"""
    idx = np.ascontiguousarray(cases[10][2][:, :1].astype(np.int32))
    d = np.ascontiguousarray(cases[10][3][:, :1])
    d[0], d[1] = 800.0, 0.0
    sigma, w, Y0 = stages[1](models[10], idx, d)
    assert sigma[0] == 1.0 and w[0, 0] == 0.0 and sigma[1] == 2.0 ** -64 and w[1, 0] == 1.0
    assert np.array_equal(Y0[:2], _map(1025, 2)[idx[:2, 0]])         # both start on their neighbour: by the rule, and as 1 y / 1


# ---- one epoch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [1, 2, 3])
def test_one_epoch_matches_the_reference(sa, stages, cases, models, dims):
    """K = 15, T = 6: 90 slots a row, more than one pass of 64 and no multiple of it"""
    epochs = stages[2]
    m = models[10, dims]
    Y_ref = _map(1025, dims)
    K, E, off = 15, 10, 1000
    idx = np.ascontiguousarray(cases[10][2][:, :K].astype(np.int32))
    _, w, _, _ = tr.smooth(cases[10][3][:, :K])
    w = np.ascontiguousarray(w)
    w[[20, 21], 0] = 1.0                                             # rate 1: these two slots fire in every epoch >= 1
    Y = tr.start(idx.astype(np.int64), w, Y_ref)
    Y[20] = Y_ref[idx[20, 0]]                                        # a query coincident in the map with its neighbour (D = 0)
    near = int(ref.draw(10, 7, np.uint64((off + 21) * K), 0, 1025))
    Y[21] = Y_ref[near] + 0.02 / np.sqrt(dims)                       # 0.02 from the vertex slot 0 draws in epoch 7 (the clip acts)
    a, b = AB
    clipped_any = 0
    for ep in (1, 7, E - 1):
        want, terms, clipped = tr.epoch(idx, w, Y, Y_ref, ep, E, a, b, seed=10, row_offset=off, return_terms=True)
        got = epochs(m, idx, w, Y, E, ep, ep + 1, seed=10, row_offset=off)
        alpha = 1.0 - ep / E
        # tests/test_umap_gpu.py's bound for epoch_kernel, without the factor 2: a term is clip(c (y_q - y_k)) in [-4, 4] with c from two
        # pow calls, a sum of <= 3 squares, a division and three products, well inside 32 eps relative; the row's sum is scaled by alpha
        bound = terms * 4 * 32 * EPS * alpha
        err = np.abs(got - want).max(1)
        print(f"dims {dims} ep {ep}: firing rows {(terms > 0).sum()}, largest err / bound {(err[terms > 0] / bound[terms > 0]).max()}")
        assert (err <= bound).all()
        assert np.array_equal(got[terms == 0], Y[terms == 0])        # a row without a firing slot stays where it is
        assert terms[20] >= 6 and terms[21] >= 6 and (ep == 1 or (terms > 0).sum() > 300)   # (at ep = 1 only a rate of 1 fires)
        clipped_any += clipped
    assert clipped_any > 0
    assert np.array_equal(epochs(m, idx, w, Y, E, 0, 1), Y)           # nothing fires in epoch 0


# ---- the invariant --------------------------------------------------------------------------------------------------------------------
def test_a_rows_result_depends_on_that_row_alone(sa, stages, cases, models):
    knn_cross, weights, epochs = stages
    m = models[10]
    Q = cases[10][1]
    E = 30
    full = sa.umap_transform(Q, m, ret_nn=True)
    Y = full["Y"]
    assert full["n_epochs"] == E and Y.shape == (333, 2) and np.isfinite(Y).all()
    # a second identical call
    assert np.array_equal(sa.umap_transform(Q, m)["Y"], Y)
    # block by block with the block's first row as row_offset
    a = sa.umap_transform(Q[:100], m, ret_nn=True)
    b = sa.umap_transform(Q[100:], m, row_offset=100, ret_nn=True)
    assert np.array_equal(np.vstack([a["Y"], b["Y"]]), Y)
    assert np.array_equal(np.vstack([a["nn"]["index"], b["nn"]["index"]]), full["nn"]["index"])
    assert np.array_equal(np.vstack([a["nn"]["distance"], b["nn"]["distance"]]), full["nn"]["distance"])
    assert not np.array_equal(sa.umap_transform(Q[100:], m)["Y"], Y[100:])          # (row_offset does number the rows)
    # knn_query's lists through the stages, the epochs in two ranges
    idx, dist = sa.knn_query(m, Q, 15)
    assert np.array_equal(idx, full["nn"]["index"]) and np.array_equal(dist, full["nn"]["distance"])
    _, w, Y0 = weights(m, idx, dist)
    assert np.array_equal(sa.umap_transform(Q, m, n_epochs=0)["Y"], Y0)             # E = 0 returns the start
    for e in (1, 11):
        assert np.array_equal(epochs(m, idx, w, epochs(m, idx, w, Y0, E, 0, e), E, e, E), Y)
    assert not np.array_equal(Y, Y0)
    # the other arguments do reach the kernel
    assert not np.array_equal(sa.umap_transform(Q, m, seed=11)["Y"], Y)
    assert not np.array_equal(sa.umap_transform(Q, m, negative_sample_rate=2)["Y"], Y)


# ---- the full run ---------------------------------------------------------------------------------------------------------------------
def test_full_run_places_new_rows_in_their_blobs(sa):
    X, lab = ref.blobs()
    fit = sa.umap(X, ret_model=True)
    with fit["model"] as m:
        assert (m.n_ref, m.d, m.dims, m.n_neighbors, m.n_epochs) == (1500, 10, 2, 15, 500) and (m.a, m.b) == (fit["a"], fit["b"])
        Q, ql = tr.full_run_queries()
        out = sa.umap_transform(Q, m)
    assert out["n_epochs"] == 166 and out["Y"].shape == (600, 2) and np.isfinite(out["Y"]).all()
    share, ratio = tr.quality(fit["Y"], lab, out["Y"], ql)
    print(f"share of queries whose nearest map neighbour carries their label {share} (floor {tr.SHARE_FLOOR}); "
          f"largest radius ratio {ratio} (ceiling {tr.RATIO_CEILING})")
    assert share >= tr.SHARE_FLOOR and ratio <= tr.RATIO_CEILING


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_library(sa, cases, models):
    X, Q, _, _ = cases[10]
    m = models[10]
    bad = Q.copy()
    bad[17, 3] = np.nan
    with pytest.raises(sa.SharpError, match=r"Xq holds NA / NaN / Inf \(row 18, column 4\)"):
        sa.umap_transform(bad, m)
    bad[17, 3] = 1e200
    with pytest.raises(sa.SharpError, match="Xq holds NA / NaN / Inf, or values so large"):
        sa.knn_query(m, bad, 15)
    badx = X.copy()
    badx[3, 0] = np.inf
    with pytest.raises(sa.SharpError, match=r"X_ref holds NA / NaN / Inf \(row 4, column 1\)"):
        sa.UmapModel(badx, _map(1025, 2), 15, 1.5, 0.9, 90)
    with pytest.raises(sa.SharpError, match="Y_ref holds NA / NaN / Inf"):
        sa.UmapModel(X, np.full((1025, 2), np.nan), 15, 1.5, 0.9, 90)
    with pytest.raises(sa.SharpError, match="ret_model is not built together with pca"):
        sa.umap(X, pca=5, ret_model=True)
    gone = sa.UmapModel(X, _map(1025, 2), 15, 1.5, 0.9, 90)
    gone.close()
    gone.close()                                                     # (closing twice is harmless)
    with pytest.raises(sa.SharpError, match="sharp_umap_transform: handle is not a live UMAP model"):
        sa.umap_transform(Q, gone)
    with pytest.raises(sa.SharpError, match="sharp_knn_cross: handle is not a live UMAP model"):
        sa.knn_query(gone, Q, 3)
    assert np.isfinite(sa.umap_transform(Q, m, n_epochs=3)["Y"]).all()               # (the library is usable after a refusal)


def test_dotc_twins(sa, cases):
    """the .C() convention (tests/test_dotc_gpu.py): same outputs as the C entries, status set on a refusal"""
    L = sa.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    I = lambda v: np.array([v], np.int32)                            # noqa: E731
    D = lambda v: np.array([v], np.float64)                          # noqa: E731
    X, Q, _, _ = cases[10]
    Q = np.ascontiguousarray(Q[:50])
    Y_ref = _map(1025, 2)
    h, st = I(0), I(-1)
    L.sharp_C_umap_model_create(*[P(v) for v in [X, D(1025), I(10), Y_ref, I(2), I(15), D(AB[0]), D(AB[1]), I(90), h, st]])
    assert st[0] == 0 and h[0] > 0
    Y, nn_i, nn_d = np.zeros((50, 2)), np.zeros((50, 15), np.int32), np.zeros((50, 15))
    tail = [I(-1), D(1.0), I(5), D(1.0), D(10.0), D(7.0), Y]
    L.sharp_C_umap_transform(*[P(v) for v in [h, Q, D(50), I(10)] + tail + [I(1), nn_i, nn_d, st]])
    with sa.UmapModel(X, Y_ref, 15, AB[0], AB[1], 90) as m:
        want = sa.umap_transform(Q, m, row_offset=7, ret_nn=True)
    assert st[0] == 0 and np.array_equal(Y, want["Y"])
    assert np.array_equal(nn_i, want["nn"]["index"]) and np.array_equal(nn_d, want["nn"]["distance"])
    keep = nn_i.copy()
    nn_i[:] = -5
    L.sharp_C_umap_transform(*[P(v) for v in [h, Q, D(50), I(10)] + tail + [I(0), nn_i, nn_d, st]])   # want_nn = 0 leaves the buffers alone
    assert st[0] == 0 and (nn_i == -5).all() and np.array_equal(Y, want["Y"]) and keep.any()
    L.sharp_C_umap_model_free(P(h), P(st))
    assert st[0] == 0
    L.sharp_C_umap_transform(*[P(v) for v in [h, Q, D(50), I(10)] + tail + [I(0), nn_i, nn_d, st]])
    buf = C.create_string_buffer(b" " * 255)
    msg, ln = (C.c_char_p * 1)(C.addressof(buf)), (C.c_int * 1)(256)
    L.sharp_C_last_error(msg, ln)
    assert st[0] == 2 and b"not a live UMAP model" in buf.value


def test_shutdown_frees_the_models_that_are_left(sa, cases, models):
    """(last in this file: the fixture's models are closed first, and closing a model twice is harmless)"""
    for m in models.values():
        m.close()
    X, Q, _, _ = cases[10]
    m = sa.UmapModel(X, _map(1025, 2), 15, AB[0], AB[1], 90)
    assert np.isfinite(sa.umap_transform(Q, m, n_epochs=2)["Y"]).all()
    sa.shutdown()
    sa.init(0)
    with pytest.raises(sa.SharpError, match="not a live UMAP model"):
        sa.umap_transform(Q, m)
    with pytest.raises(sa.SharpError, match="not a live UMAP model"):
        m.close()
    with sa.UmapModel(X, _map(1025, 2), 15, AB[0], AB[1], 90) as again:              # (and new models work after the re-init)
        assert np.isfinite(sa.umap_transform(Q, again, n_epochs=2)["Y"]).all()
