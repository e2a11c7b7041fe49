"""Diffusion maps and pseudotime on the GPU against tests/_diffmap_ref.py: the transition scaling, the extraction of a
component, the thick-restart solver with §15's bounds (derived, not tuned), the outcome under a cap that is too small, reproducibility,
the pseudotime stage and the whole call.  The shapes are the smallest at which each kernel can still go wrong."""
import warnings

import numpy as np
import pytest

import _diffmap_ref as dr
import _umap_spectral_ref as sr

pytestmark = pytest.mark.gpu
EPS = dr.EPS


@pytest.fixture(scope="module")
def sharp():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


def _solve(sharp, name, n_comps, density=True, **kw):
    return sharp.diffmap_graph(*dr.case(name), n_comps=n_comps, density_normalize=density, tol=dr.TOL, **kw)


# ---- transitions ----------------------------------------------------------------------------------------------------------------------
def _depth(length):
    """roundings on the way of a row sum of non-negative terms: a lane adds its ceil(L / 64) terms one after the other (the first to 0,
    exactly), six butterfly steps fold the lanes"""
    return (np.asarray(length) + 63) // 64 - 1 + 6


@pytest.mark.parametrize("name", ["slab14", "hub", "slab_odd"])
@pytest.mark.parametrize("density", [True, False])
def test_transitions(sharp, name, density):
    """a and z within (row length + 3) eps relative of the long-double reference.  Derivation, with u = eps / 2 and d(L) = _depth(L): every
    sum is of non-negative terms, so q_j carries at most d(L_j) u.  A term W_ij / q_j then carries (d(L_j) + 1) u, their sum d(L_i) u more,
    the division by q_i another d(L_i) + 1: z_i within (max_j d(L_j) + 2 d(L_i) + 2) u.  a_i = 1 / (q_i sqrt(z_i)): d(L_i) u for q_i, half
    of z's plus one for the root, one for the product, one for the division.  Without density normalisation z = q and a = 1 / sqrt(q):
    d(L_i) u and d(L_i) / 2 + 2 u.  With rows of at least 14 entries and none beyond 688 all of these are below (L_i + 3) eps, which the
    first assertion checks before the bound is used."""
    from sharp_amd.diffmap import _transitions

    rp, col, val = dr.case(name)
    L = np.diff(rp)
    d, dmax = _depth(L), _depth(L.max())
    zb = (dmax + 2 * d + 2) / 2 if density else d / 2
    ab = (d / 2 + zb / 2 + 1.5) if density else (d / 4 + 1)                    # (both in units of eps)
    assert (zb <= L + 3).all() and (ab <= L + 3).all()
    a, z = _transitions(rp, col, val, density)
    al, zl = dr.transitions(rp, col, val, density, np.longdouble)
    ea, ez = np.abs(a - al) / al, np.abs(z - zl) / zl
    print(f"{name} density {density}: worst a {float(ea.max() / EPS):.2f} eps, worst z {float(ez.max() / EPS):.2f} eps")
    assert (ea <= (L + 3) * EPS).all() and (ez <= (L + 3) * EPS).all()


def test_transitions_of_an_empty_row(sharp):
    from sharp_amd.diffmap import _transitions

    rp, col, val = dr.with_empty_row(*dr.case("small"))
    for density in (True, False):
        a, z = _transitions(rp, col, val, density)
        assert a[5] == 0.0 and z[5] == 0.0 and (a[np.arange(20) != 5] > 0).all()


# ---- the component --------------------------------------------------------------------------------------------------------------------
def _same_component(got, want):
    assert got[0] == want[0] and got[1] == want[1]
    for g, w in zip(got[2], want[2]):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert np.array_equal(got[3], want[3])


def test_component_extraction(sharp):
    from sharp_amd.diffmap import _component

    two = dr.case("two_slabs")
    _same_component(_component(*two, 4), dr.component(*two))                    # the larger, without a root
    assert _component(*two, 4)[0] == 512
    _same_component(_component(*two, 4, root=3), dr.component(*two, root=3))    # the smaller, by a root inside it
    halves = dr.two_halves()
    got = _component(*halves, 4)
    _same_component(got, dr.component(*halves))
    assert got[0] == 0                                                        # the tie goes to the smaller label
    one = dr.case("slab_odd")
    _same_component(_component(*one, 4), dr.component(*one))                    # a connected graph comes back as it is
    with pytest.raises(sharp.SharpError, match="holds 3 rows, fewer than n_comps \\+ 2"):
        _component(*sr.edges_and_triangle(), 4)
    with pytest.raises(sharp.SharpError, match="holds 3 rows, fewer than n_comps \\+ 2"):
        sharp.diffmap_graph(*sr.edges_and_triangle(), n_comps=4)


def test_empty_row_is_left_out(sharp):
    rp, col, val = dr.with_empty_row(*dr.case("small"))
    from sharp_amd.diffmap import _component

    _same_component(_component(rp, col, val, 4), dr.component(rp, col, val))
    with pytest.warns(RuntimeWarning, match="2 connected components; the one of 19 cells was solved and 1 cells are left out"):
        dm = sharp.diffmap_graph(rp, col, val, n_comps=4, tol=dr.TOL)
    assert np.isnan(dm["evecs"][5]).all() and not dm["in_component"][5] and dm["in_component"].sum() == 19
    assert np.isfinite(np.delete(dm["evecs"], 5, 0)).all() and dm["components"] == 2 and dm["component_size"] == 19
    assert np.isinf(sharp.dpt(dm, root=0, n_dcs=4)[5])


# ---- the solver -----------------------------------------------------------------------------------------------------------------------
def _norms(V):
    """the columns' 2-norms summed in long double: numpy adds the rows of a C-ordered matrix one after the other in fp64, which drifts by
    tens of eps on a column of 1 025 nearly equal values (q0 of the path graph)"""
    return np.sqrt((V.astype(np.longdouble) ** 2).sum(0)).astype(np.float64)


def _check_pairs(dm, T, q0l, L, lam, U, gap, tol):
    """§15's bounds on every non-trivial pair, and the trivial one; returns the vector bounds (b[0]: q0's)"""
    n, nc = dm["evecs"].shape
    V, theta = dm["evecs"], dm["evals"]
    assert theta[0] == 1.0
    assert (np.abs(V[:, 0] - q0l) <= (L + 3) * EPS * q0l).all()               # the transitions' bound
    res = np.linalg.norm(T @ V - V * theta, axis=0)
    print(f"steps {dm['steps']} restarts {dm['restarts']} largest residual {dm['residual'].max():.2e} (numpy {res.max():.2e})")
    assert (res <= tol + 64 * EPS).all() if dm["converged"] else True
    assert (np.abs(res - dm["residual"]) <= 1e-13).all()
    assert (np.abs(_norms(V) - 1.0) <= 8 * EPS).all()
    assert np.array_equal(V, sr.sign_rule(V))                                 # the sign rule
    r = dm["residual"][1:]
    b = np.concatenate([[float(((L + 3) * EPS).max())], sr.vector_bound(r, gap[1:], n)])
    if dm["converged"]:
        assert (np.abs(theta[1:] - lam[1:]) <= r + n * EPS).all()
        assert (np.linalg.norm(V[:, 1:] - U[:, 1:], axis=0) <= b[1:]).all()
        G = np.abs(V.T @ V)
        np.fill_diagonal(G, 0.0)
        assert (G <= b[:, None] + b[None, :]).all()                           # |v_j . v_k| and |v_j . q0|
    return b


@pytest.mark.parametrize("name,n_comps", dr.SOLVER_CASES)
def test_solver(sharp, name, n_comps):
    dm = _solve(sharp, name, n_comps)
    T, q0, lam, U, gap = dr.dense(name, n_comps)
    rp, col, val = dr.case(name)
    zl = dr.transitions(rp, col, val, True, np.longdouble)[1]
    q0l = (np.sqrt(zl) / np.sqrt((zl).sum())).astype(np.float64)
    assert dm["converged"] and dm["components"] == 1 and dm["component_size"] == T.shape[0] and dm["in_component"].all()
    assert dm["steps"] <= dr.MAX_MATVECS and dm["density_normalize"] is True
    _check_pairs(dm, T, q0l, np.diff(rp), lam, U, gap, dr.TOL)
    emu = dr.emulated(name, n_comps)
    if (name, n_comps) == dr.RESTART_CASE:
        # without the restart this case cannot converge inside m columns
        assert emu["restarts"] >= 2 and dm["restarts"] >= 1 and dm["steps"] > dr.basis(n_comps - 1)
    if name == "small":
        assert dm["steps"] == 19 < dr.basis(n_comps - 1) and dm["restarts"] == 0   # the Krylov space is exhausted first


def test_solver_without_density_normalisation_agrees_with_the_spectral_start(sharp):
    from sharp_amd.umap import _spectral

    rp, col, val = dr.case("slab14")
    dm = _solve(sharp, "slab14", 4, density=False)
    sp = _spectral(rp, col, val, dims=3, tol=1e-10)
    T, q0, lam, U, gap = dr.dense("slab14", 4, False)
    assert dm["converged"] and sp["outcome"] == 0 and dm["density_normalize"] is False
    n = T.shape[0]
    bound = sr.vector_bound(dm["residual"][1:], gap[1:], n) + sr.vector_bound(sp["residual"], gap[1:], n)
    assert (np.linalg.norm(dm["evecs"][:, 1:] - sp["V"], axis=0) <= bound).all()
    assert (np.abs(dm["evals"][1:] - sp["theta"]) <= dm["residual"][1:] + sp["residual"] + 2 * n * EPS).all()
    _check_pairs(dm, T, q0, np.diff(rp), lam, U, gap, dr.TOL)


def test_not_converged_under_a_small_cap(sharp):
    emu = dr.emulated("path", 16, True, dr.PATH_CAP)
    assert emu["outcome"] == 2
    with pytest.warns(RuntimeWarning, match="not converged after 300 operator applications: the largest residual is"):
        dm = _solve(sharp, "path", 16, max_matvecs=dr.PATH_CAP)
    assert dm["converged"] is False and dm["steps"] == dr.PATH_CAP and dm["restarts"] >= 1
    assert dm["residual"].max() > dr.TOL
    T, _ = dr.operator(*dr.case("path"))
    V, theta = dm["evecs"], dm["evals"]
    assert (np.abs(_norms(V) - 1.0) <= 8 * EPS).all()
    assert (np.abs(np.linalg.norm(T @ V - V * theta, axis=0) - dm["residual"]) <= 1e-13).all()


# ---- reproducibility ------------------------------------------------------------------------------------------------------------------
def _same_map(a, b):
    for key in ("evals", "evecs", "residual", "in_component"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    for key in ("converged", "steps", "restarts", "components", "component_size", "density_normalize"):
        assert a[key] == b[key], key


def test_two_calls_and_three_doors_give_the_same_bits(sharp):
    from sharp_amd.umap import _graph

    X = sr.slab()
    a = sharp.diffmap(X, n_comps=10, ret_nn=True)
    _same_map(a, sharp.diffmap(X, n_comps=10))
    b = sharp.diffmap_neighbors(a["nn"]["index"], a["nn"]["distance"], n_comps=10)
    _same_map(a, b)
    rp, col, val = _graph(a["nn"]["index"], a["nn"]["distance"])[:3]
    _same_map(a, sharp.diffmap_graph(rp, col, val, n_comps=10))
    assert a["converged"] and a["evecs"].shape == (1025, 10)


# ---- pseudotime -----------------------------------------------------------------------------------------------------------------------
def _dpt_bound(n_dcs, normalize):
    """relative, between two fp64 evaluations of the formula on the same inputs: a term t = w (a - b) carries 2 u, its square 5 u, the sum
    of n_dcs - 1 non-negative terms n_dcs - 2 more, the root halves that and adds one: ((n_dcs + 3) / 2 + 1) u each side, twice that
    between the two, and with normalize the same again for the divisor plus one for the division"""
    b = (n_dcs + 5) * EPS / 2
    return 2 * b + EPS if normalize else b


@pytest.mark.parametrize("n_dcs", [2, 10, 16])
@pytest.mark.parametrize("normalize", [True, False])
def test_dpt_stage(sharp, n_dcs, normalize):
    T, q0, lam, U, gap = dr.dense("slab14", 16)
    V = U.copy()
    outside = np.array([11, 500, 1024])
    V[outside] = np.nan
    dm = {"evals": lam, "evecs": V}
    roots = np.array([0, 77, 300, 640, 1023])
    want = dr.dpt(lam, V, roots, n_dcs, normalize)
    many = sharp.dpt(dm, roots=roots, n_dcs=n_dcs, normalize=normalize)
    one = sharp.dpt(dm, root=77, n_dcs=n_dcs, normalize=normalize)
    assert many.shape == (1025, 5) and one.shape == (1025,)
    assert np.array_equal(one, many[:, 1])                                    # five roots in one call are five calls
    assert np.isinf(many[outside]).all() and np.isfinite(np.delete(many, outside, 0)).all()
    assert (many[roots, np.arange(5)] == 0.0).all()                           # a root's own pseudotime
    fin = np.isfinite(want)
    assert (np.abs(many[fin] - want[fin]) <= _dpt_bound(n_dcs, normalize) * want[fin]).all()
    if normalize:
        assert (np.delete(many, outside, 0).max(0) == 1.0).all()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def _rank_correlation(a, b):
    ra, rb = np.argsort(np.argsort(a)).astype(float), np.argsort(np.argsort(b)).astype(float)
    return float(np.corrcoef(ra, rb)[0, 1])


def test_end_to_end_pseudotime_of_the_slab(sharp):
    """dpt(diffmap(slab), root = argmin x0) against the dense eigenpairs of the graph the call built.  The bound carries the eigenpair
    bounds through w = lambda / (1 - lambda): |dpt - dpt_ref| <= sum_l (|dw_l| |psi_l(r) - psi_l(i)| + w_l (b_l + b_l)) with dw_l over
    [lambda_l +- (r_l + n eps)] and b_l the Davis-Kahan bound of vector l (it bounds every component), plus the formula's own rounding."""
    from sharp_amd.umap import _graph

    X = sr.slab()
    n_comps, n_dcs = 15, 10
    dm = sharp.diffmap(X, n_comps=n_comps, tol=dr.TOL, ret_nn=True)
    assert dm["converged"] and dm["components"] == 1
    rp, col, val = _graph(dm["nn"]["index"], dm["nn"]["distance"])[:3]
    T, _ = dr.operator(rp, col, val)
    lam, U, gap = dr.dense_of(T, n_comps)
    n = T.shape[0]
    root = int(np.argmin(X[:, 0]))
    got = sharp.dpt(dm, root=root, n_dcs=n_dcs, normalize=False)
    want = dr.dpt(lam, U, root, n_dcs, False)[:, 0]
    ls = slice(1, n_dcs)
    delta = dm["residual"][ls] + n * EPS
    w = lam[ls] / (1 - lam[ls])
    dw = np.maximum(np.abs((lam[ls] + delta) / (1 - lam[ls] - delta) - w), np.abs((lam[ls] - delta) / (1 - lam[ls] + delta) - w))
    b = sr.vector_bound(dm["residual"][ls], gap[ls], n)
    bound = (np.abs(U[root, ls][None, :] - U[:, ls]) * dw[None, :]).sum(1) + (2 * w * b).sum() + _dpt_bound(n_dcs, False) * want
    err = np.abs(got - want)
    rho = _rank_correlation(sharp.dpt(dm, root=root, n_dcs=n_dcs), X[:, 0])
    print(f"largest error {err.max():.2e} against a bound of {bound[err.argmax()]:.2e}; rank correlation with the long axis {rho:.4f} "
          f"(dense reference {_rank_correlation(want, X[:, 0]):.4f})")
    assert (err <= bound).all() and got[root] == 0.0


def test_end_to_end_on_two_slabs(sharp):
    from sharp_amd.umap import _graph

    X = sr.two_slabs()
    with pytest.warns(RuntimeWarning, match="2 connected components; the one of 513 cells was solved and 512 cells are left out"):
        dm = sharp.diffmap(X, n_comps=10, ret_nn=True)
    inside = dm["in_component"]
    assert inside.sum() == 513 and inside[512:].all() and dm["components"] == 2 and dm["component_size"] == 513
    assert np.isnan(dm["evecs"][~inside]).all() and np.isfinite(dm["evecs"][inside]).all()
    t = sharp.dpt(dm, root=600)
    assert np.isinf(t[~inside]).all() and np.isfinite(t[inside]).all() and t[600] == 0.0 and t[inside].max() == 1.0
    with pytest.raises(sharp.SharpError, match="outside the component"):
        sharp.dpt(dm, root=3)
    # the component alone gives the same bits
    rp, col, val = _graph(dm["nn"]["index"], dm["nn"]["distance"])[:3]
    _, _, sub, new_id = dr.component(rp, col, val)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        alone = sharp.diffmap_graph(*sub, n_comps=10)
    assert np.array_equal(alone["evecs"], dm["evecs"][inside]) and np.array_equal(alone["evals"], dm["evals"])
    assert np.array_equal(sharp.dpt(alone, root=int(new_id[600])), t[inside])
    # a root in the smaller slab turns the choice round
    with pytest.warns(RuntimeWarning, match="the one of 512 cells was solved and 513 cells are left out"):
        dm0 = sharp.diffmap(X, n_comps=10, root=3)
    assert dm0["in_component"][:512].all() and not dm0["in_component"][512:].any()
