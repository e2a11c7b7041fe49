"""UMAP's spectral start on the MI355X against the numpy specification (tests/_umap_spectral_ref.py): the connected
components, the eigensolver on its own input (a CSR built by the reference, so the solver inherits no other stage's rounding), the three
outcomes, and the drivers' init = "normlaplacian" with its fallbacks.  Every bound is derived where it is used; none is tuned."""
import ctypes as C
import warnings

import numpy as np
import pytest

import _umap_ref as ref
import _umap_spectral_ref as sr

pytestmark = pytest.mark.gpu
EPS = sr.EPS
TOL = sr.TOL


@pytest.fixture(scope="module")
def sa():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


@pytest.fixture(scope="module")
def stages():
    from sharp_amd.umap import _components, _graph, _spectral

    return _graph, _components, _spectral


# ---- 1. components --------------------------------------------------------------------------------------------------------------------
def test_components_of_a_shuffled_path_in_few_sweeps(sa, stages):
    """A plain min-label sweep needs as many sweeps as the path is long.  Here a sweep hooks every tree's root onto the smallest root
    beside it and flattens the trees: the trees of a path are stretches of it, a stretch survives a sweep as a root only when both
    stretches beside it carry larger labels, no two survivors are adjacent, so s trees become at most ceil(s / 2): 1 025 -> 1 takes at
    most ceil(log2 1025) = 11 sweeps, and one more finds nothing to do.  One `umap_components` timer is recorded per sweep."""
    from sharp_amd import device

    _, components, _ = stages
    rp, col, _ = sr.case("path")
    n = rp.size - 1
    device.profile(True)
    try:
        label, count = components(rp, col)
        sweeps = device.profile_table()["umap_components"][1]
    finally:
        device.profile(False)
    print("sweeps on the shuffled path:", sweeps)
    assert n == 1025 and count == 1 and (label == 0).all()
    assert sweeps <= int(np.ceil(np.log2(n))) + 1


def _with_empty_row():
    """a path on 70 shuffled vertices from which vertex 37 is cut out: its row is empty"""
    rp, col, _ = sr.path_graph(70, seed=8)
    row = np.repeat(np.arange(70), np.diff(rp))
    keep = (row != 37) & (col != 37)
    nrp = np.zeros(71, np.int64)
    np.add.at(nrp, row[keep] + 1, 1)
    return np.cumsum(nrp), col[keep]


@pytest.mark.parametrize("name", ["two_slabs", "edges_and_triangle", "empty_row"])
def test_components_match_union_find(sa, stages, name):
    _, components, _ = stages
    rp, col = {"two_slabs": lambda: sr.case("two_slabs")[:2], "edges_and_triangle": lambda: sr.edges_and_triangle()[:2],
               "empty_row": _with_empty_row}[name]()
    want, want_count = sr.components(rp, col)
    label, count = components(rp, col)
    assert count == want_count == {"two_slabs": 2, "edges_and_triangle": 513, "empty_row": 3}[name]
    assert np.array_equal(label, want)
    if name == "empty_row":
        assert rp[38] == rp[37] and label[37] == 37


# ---- 2. the solver --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dims", [("slab14", 1), ("slab14", 2), ("slab14", 3), ("slab64", 3), ("hub", 3), ("ribbon", 3)])
def test_solver_against_dense_eigh(sa, stages, name, dims):
    _, _, spectral = stages
    rp, col, val = sr.case(name)
    n = rp.size - 1
    M, q0, lam, U, gap = sr.dense(name)
    lam, U, gap = lam[:dims], U[:, :dims], gap[:dims]
    got = spectral(rp, col, val, dims, TOL, sr.MAX_STEPS)
    assert got["outcome"] == 0 and got["components"] == 1 and dims <= got["steps"] <= sr.MAX_STEPS
    V, theta = got["V"], got["theta"]
    # the true residual against the reference's M: <= tol plus the rounding of two evaluations of a unit vector's image (64 eps)
    r = np.linalg.norm(M @ V - V * theta, axis=0)
    print(f"{name} dims {dims}: steps {got['steps']}, theta {theta}, residual {r} (reported {got['residual']})")
    assert (r <= TOL + 64 * EPS).all()
    assert (np.abs(r - got["residual"]) <= 1e-13).all()
    assert (np.abs(theta - lam) <= r + n * EPS).all()
    # Davis-Kahan, with n eps for eigh's own error
    bound = sr.vector_bound(r, gap, n)
    err = np.linalg.norm(V - U, axis=0)
    print(f"    |theta - lambda| {np.abs(theta - lam)}, ||v - u|| {err}, bound {bound}")
    assert (err <= bound).all()
    assert (np.abs(np.linalg.norm(V, axis=0) - 1.0) <= 8 * EPS).all()
    # orthogonality follows from the vectors' own errors: |v_j . v_k| = |(v_j - u_j) . v_k + u_j . (v_k - u_k)| <= b_j + b_k
    b0 = sr.vector_bound(np.linalg.norm(M @ q0 - q0), 1.0 - lam[0], n)
    for j in range(dims):
        assert abs(V[:, j] @ q0) <= bound[j] + b0
        for k in range(j):
            assert abs(V[:, j] @ V[:, k]) <= bound[j] + bound[k]
    assert np.array_equal(sr.sign_rule(V), V)
    for j in range(dims):
        assert V[np.abs(V[:, j]).argmax(), j] > 0
    again = spectral(rp, col, val, dims, TOL, sr.MAX_STEPS)
    assert np.array_equal(again["V"], V) and np.array_equal(again["theta"], theta) and np.array_equal(again["residual"], got["residual"])
    assert again["steps"] == got["steps"]


def test_outcome_not_connected_leaves_the_outputs(sa, stages):
    _, _, spectral = stages
    rp, col, val = sr.case("two_slabs")
    V = np.full((rp.size - 1, 3), np.nan)
    got = spectral(rp, col, val, 3, TOL, sr.MAX_STEPS, V=V)
    assert got["outcome"] == 1 and got["components"] == 2 and got["steps"] == 0
    assert np.isnan(V).all() and (got["theta"] == 0).all() and (got["residual"] == 0).all()


def test_outcome_not_converged_leaves_v(sa, stages):
    _, _, spectral = stages
    rp, col, val = sr.case("path")
    V = np.full((rp.size - 1, 3), np.nan)
    got = spectral(rp, col, val, 3, TOL, 40, V=V)
    print("the path after 40 steps: residual estimates", got["residual"])
    assert got["outcome"] == 2 and got["components"] == 1 and got["steps"] == 40
    assert got["residual"].max() > TOL and np.isfinite(got["residual"]).all()
    assert np.isnan(V).all() and (got["theta"] == 0).all()


# ---- 3. the drivers -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slab_start(sa, stages):
    """the slab, its lists from the GPU, the GPU's CSR of them and the stage's solve at the library's defaults"""
    graph, _, spectral = stages
    X = sr.slab()
    idx, d = sa.knn(X, 14)
    rp, col, val = graph(idx, d)[:3]
    return X, idx, d, (rp, col, val), {dims: spectral(rp, col, val, dims) for dims in (2, 3)}


def test_umap_normlaplacian_is_the_given_matrix_start(sa, slab_start):
    X, idx, d, _, solved = slab_start
    S = solved[2]
    assert S["outcome"] == 0 and S["components"] == 1 and (S["residual"] <= 1e-6).all()      # the defaults: tol 1e-6, 400 steps
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)               # no fallback, no warning
        r = sa.umap(X, n_epochs=30, init="normlaplacian", ret_nn=True)
        rn = sa.umap_neighbors(idx, d, n_epochs=30, init="normlaplacian")
    assert np.array_equal(r["nn"]["index"], idx) and np.array_equal(r["nn"]["distance"], d)
    want = sa.umap(X, n_epochs=30, init=S["V"])
    assert np.array_equal(r["Y"], want["Y"]) and np.isfinite(r["Y"]).all()
    assert np.array_equal(rn["Y"], sa.umap_neighbors(idx, d, n_epochs=30, init=S["V"])["Y"]) and np.array_equal(rn["Y"], r["Y"])
    for out in (r, rn):
        assert out["init"] == {"requested": "normlaplacian", "used": "normlaplacian", "components": 1, "steps": S["steps"],
                               "residual": S["residual"].max()}
    assert "init" not in want and "init" not in sa.umap(X, n_epochs=0, init="random")
    assert not np.array_equal(r["Y"], sa.umap(X, n_epochs=30)["Y"])  # (it is not the PCA start)


@pytest.mark.parametrize("dims", [2, 3])
def test_start_is_the_scaled_dense_eigenvectors(sa, slab_start, dims):
    """n_epochs = 0 returns the start.  With b_k the Davis-Kahan bound of coordinate k (every component of v - u is within it), the
    map y = 10 (v - min v) / (max v - min v) moves by at most 10 (2 b / w' + 2 b / w') with w' = w - 2 b the smallest range the
    returned vector can have, w the range of the reference's: numerator and range each change by at most 2 b, and the quotient lies in
    [0, 1].  64 eps covers the map's own rounding on values up to 10."""
    X, idx, d, (rp, col, val), solved = slab_start
    S = solved[dims]
    n = X.shape[0]
    M, q0 = sr.operator(rp, col, val)
    w, Q = np.linalg.eigh(M)
    w, Q = w[::-1], Q[:, ::-1]
    U = sr.sign_rule(Q[:, 1:dims + 1])
    gap = np.array([min(w[j] - w[j + 1], w[j - 1] - w[j]) for j in range(1, dims + 1)])
    r = np.linalg.norm(M @ S["V"] - S["V"] * S["theta"], axis=0)
    b = sr.vector_bound(r, gap, n)
    assert (gap >= 1e-3).all() and (sr.sign_margin(U) > 2 * b).all()
    want = ref.scale_start(U)
    rng = U.max(0) - U.min(0)
    tol = 10.0 * 4.0 * b / (rng - 2.0 * b) + 64 * EPS * 10.0
    for out in (sa.umap(X, n_components=dims, n_epochs=0, init="normlaplacian"),
                sa.umap_neighbors(idx, d, n_components=dims, n_epochs=0, init="normlaplacian")):
        err = np.abs(out["Y"] - want).max(0)
        print(f"dims {dims}: largest |Y - scale_start(U)| per coordinate {err}, bound {tol}")
        assert (err <= tol).all()
        assert np.array_equal(out["Y"], ref.scale_start(S["V"]))     # and it is the stage's V through the common mapping, to the bit
        assert out["init"]["used"] == "normlaplacian"


def test_a_graph_in_pieces_falls_back(sa):
    X = sr.two_slabs()
    with pytest.warns(RuntimeWarning, match="fell back to \"pca\": the graph has 2 connected components"):
        r = sa.umap(X, n_epochs=30, init="normlaplacian", ret_nn=True)
    assert r["init"]["requested"] == "normlaplacian" and r["init"]["used"] == "pca" and r["init"]["components"] == 2
    assert r["init"]["steps"] == 0
    assert np.array_equal(r["Y"], sa.umap(X, n_epochs=30, init="pca")["Y"])
    idx, d = r["nn"]["index"], r["nn"]["distance"]
    with pytest.warns(RuntimeWarning, match="fell back to \"random\""):
        rn = sa.umap_neighbors(idx, d, n_epochs=30, init="normlaplacian", seed=7)
    assert rn["init"]["used"] == "random" and rn["init"]["components"] == 2
    assert np.array_equal(rn["Y"], sa.umap_neighbors(idx, d, n_epochs=30, init="random", seed=7)["Y"])
    assert not np.array_equal(rn["Y"], sa.umap_neighbors(idx, d, n_epochs=30, init="random", seed=8)["Y"])


def test_visualization_sharp_forwards_the_init(sa, slab_start):
    """with given lists and this init no x1 is built: a result that holds nothing to build it from is enough"""
    X, idx, d, _, _ = slab_start
    n = X.shape[0]
    nb = {"index": idx, "distance": d, "squared": False, "w": 2, "n": n}
    v = sa.visualization_SHARP({"viE": np.full((n, 1), np.nan)}, method="umap", neighbors=nb, init="normlaplacian", plot=False, n_epochs=30)
    want = sa.umap_neighbors(idx, d, n_epochs=30, init="normlaplacian")
    assert np.array_equal(v["Y"], want["Y"]) and v["init"] == want["init"]


# ---- 4. the .C() twins ------------------------------------------------------------------------------------------------------------------
def test_dotc_twins(sa, stages, slab_start):
    """the .C() convention (tests/test_umap_gpu.py): the outputs of the C entries, the status set on a refusal"""
    _, components, spectral = stages
    L = sa.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    I = lambda v: np.array([v], np.int32)                            # noqa: E731
    D = lambda v: np.array([v], np.float64)                          # noqa: E731
    X, idx, d, (rp, col, val), solved = slab_start
    n = X.shape[0]
    rpd = rp.astype(np.float64)
    label, count, st = np.zeros(n, np.int32), D(-1), I(-1)
    L.sharp_C_umap_components(*[P(v) for v in [rpd, col, D(n), label, count, st]])
    assert st[0] == 0 and count[0] == 1 and (label == 0).all()
    V, theta, res, steps, comp, outcome = np.zeros((n, 2)), np.zeros(2), np.zeros(2), I(-1), D(-1), I(-1)
    L.sharp_C_umap_spectral(*[P(v) for v in [rpd, col, val, D(n), I(2), D(0.0), I(0), V, theta, res, steps, comp, outcome, st]])
    S = solved[2]
    assert st[0] == 0 and outcome[0] == 0 and comp[0] == 1 and steps[0] == S["steps"]
    assert np.array_equal(V, S["V"]) and np.array_equal(theta, S["theta"]) and np.array_equal(res, S["residual"])
    # init = 3 through sharp_C_umap_neighbors, then the info of that call
    Y, ab = np.zeros((n, 2)), np.zeros(2)
    opt = [I(2), I(30), D(1.0), D(0.01), D(1.0), ab, I(5), D(1.0)]
    L.sharp_C_umap_neighbors(*[P(v) for v in [idx, d, D(n), I(14), I(0)] + opt + [I(3), np.zeros(1), D(10.0), Y, st]])
    assert st[0] == 0
    req, used, cmp2, stp, rs = I(-1), I(-1), D(-1), I(-1), D(-1)
    L.sharp_C_umap_init_info(*[P(v) for v in [req, used, cmp2, stp, rs, st]])
    assert st[0] == 0 and (req[0], used[0], cmp2[0], stp[0], rs[0]) == (3, 3, 1, S["steps"], S["residual"].max())
    assert np.array_equal(Y, sa.umap_neighbors(idx, d, n_epochs=30, init=S["V"])["Y"])
    L.sharp_C_umap_init_info(*[P(v) for v in [req, used, cmp2, stp, rs, st]])
    assert (req[0], used[0], cmp2[0], stp[0], rs[0]) == (2, 2, 0, 0, 0)          # (the info is the last call's)
    # a call with another init reports that init and no spectral stage
    sa.umap_neighbors(idx, d, n_epochs=0, init="random")
    L.sharp_C_umap_init_info(*[P(v) for v in [req, used, cmp2, stp, rs, st]])
    assert (req[0], used[0], cmp2[0], stp[0], rs[0]) == (1, 1, 0, 0, 0)
    # refusals: the status and the message
    buf = C.create_string_buffer(b" " * 255)
    msg, ln = (C.c_char_p * 1)(C.addressof(buf)), (C.c_int * 1)(256)
    L.sharp_C_umap_spectral(*[P(v) for v in [rpd, col, val, D(n), I(4), D(0.0), I(0), V, theta, res, steps, comp, outcome, st]])
    L.sharp_C_last_error(msg, ln)
    assert st[0] == 2 and b"n_components must be 1, 2 or 3" in buf.value
    bad = col.copy()
    bad[5] = n
    L.sharp_C_umap_components(*[P(v) for v in [rpd, bad, D(n), label, count, st]])
    assert st[0] == 2
