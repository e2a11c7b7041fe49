"""Diffusion maps and pseudotime without a GPU: the premises of the numpy reference that the GPU tests compare against
(tests/_diffmap_ref.py), asserted so that the reference alone stays within every condition those comparisons rely on; the emulation of
the thick-restart recurrence against the library's constants; the refusals that happen before the library; the new entries' export."""
import ctypes as C

import numpy as np
import pytest

import _diffmap_ref as dr
import _umap_spectral_ref as sr


@pytest.fixture(scope="module")
def sharp():
    import os

    import __graft_entry__ as g

    import sharp_amd

    if not os.path.exists(sharp_amd.so_path()):
        g.build()
    return sharp_amd


# ---- 1. the operator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["slab14", "hub", "ribbon", "small", "slab_odd"])
@pytest.mark.parametrize("density", [True, False])
def test_T_is_symmetric_and_fixes_sqrt_z(name, density):
    rp, col, val = dr.case(name)
    T, q0 = dr.operator(rp, col, val, density)
    assert np.abs(T - T.T).max() == 0.0
    assert np.linalg.norm(T @ q0 - q0) <= 64 * dr.EPS
    assert abs(np.linalg.norm(q0) - 1.0) <= 4 * dr.EPS and (q0 > 0).all()
    a, z = dr.transitions(rp, col, val, density)
    al, zl = dr.transitions(rp, col, val, density, np.longdouble)
    assert (np.abs(a - al) <= 64 * dr.EPS * al).all() and (np.abs(z - zl) <= 64 * dr.EPS * zl).all()


@pytest.mark.parametrize("name", ["slab14", "hub", "ribbon"])
def test_without_density_normalisation_T_is_the_spectral_starts_M(name):
    rp, col, val = dr.case(name)
    T, q0 = dr.operator(rp, col, val, False)
    M, s0 = sr.operator(rp, col, val)
    assert np.array_equal(T, M) and np.array_equal(q0, s0)


def test_shapes_of_the_transition_cases():
    assert np.diff(dr.case("hub")[0])[0] == 688 == 10 * 64 + 48       # eleven passes of 64 lanes
    n = dr.case("slab_odd")[0].size - 1
    assert n == 1023 and n % 4 and n % 64 and n % 256
    assert sr.components(*dr.case("slab_odd")[:2])[1] == 1
    for name in ("slab14", "slab_odd", "hub"):                       # the bound (row length + 3) eps of the GPU test needs rows of >= 14
        assert np.diff(dr.case(name)[0]).min() >= 14


# ---- 2. the component -----------------------------------------------------------------------------------------------------------------
def test_component_choice_and_tie_rule():
    rp, col, val = dr.case("two_slabs")
    lab, count, (srp, scol, sval), new_id = dr.component(rp, col, val)
    assert count == 2 and lab == 512 and srp.size - 1 == 513         # the second slab is the larger one
    lab0, _, (srp0, _, _), new0 = dr.component(rp, col, val, root=3)
    assert lab0 == 0 and srp0.size - 1 == 512 and (new0[:512] == np.arange(512)).all() and (new0[512:] == -1).all()
    W = dr.dense_w(rp, col, val)
    assert np.array_equal(dr.dense_w(srp, scol, sval), W[512:, 512:])
    rp, col, val = dr.two_halves()
    lab, count, (srp, _, _), new_id = dr.component(rp, col, val)
    assert count == 2 and lab == 0 and srp.size - 1 == 20 and (new_id[0::2] == np.arange(20)).all() and (new_id[1::2] == -1).all()
    rp, col, val = sr.edges_and_triangle()
    lab, count, (srp, _, _), _ = dr.component(rp, col, val)
    assert count == 513 and srp.size - 1 == 3 < 4 + 2                # refused at n_comps = 4
    rp, col, val = dr.with_empty_row(*dr.case("small"))
    lab, count, (srp, _, _), new_id = dr.component(rp, col, val)
    assert count == 2 and rp[5] == rp[6] and new_id[5] == -1 and srp.size - 1 == 19


# ---- 3. the solver's premises ---------------------------------------------------------------------------------------------------------
def test_constants():
    assert [(dr.basis(k), dr.keep(k)) for k in (1, 3, 9, 15, 31, 63)] == [(32, 8), (32, 8), (48, 16), (64, 24), (112, 48), (208, 96)]
    for k in range(1, 64):
        assert k < dr.keep(k) <= 96 and dr.basis(k) - dr.keep(k) >= k + 1


@pytest.mark.parametrize("name,n_comps", dr.SOLVER_CASES)
@pytest.mark.parametrize("density", [True, False])
def test_emulation_converges_with_twice_the_headroom(name, n_comps, density):
    got = dr.emulated(name, n_comps, density)
    T, q0, lam, U, gap = dr.dense(name, n_comps, density)
    n, k = T.shape[0], n_comps - 1
    print(f"{name} n_comps {n_comps} density {density}: m {dr.basis(k)} p {dr.keep(k)} steps {got['steps']} restarts {got['restarts']} "
          f"largest residual {got['residual'].max():.2e} smallest gap {gap[1:].min():.2e}")
    assert got["outcome"] == 0 and 2 * got["steps"] <= dr.MAX_MATVECS
    assert (got["residual"] <= dr.TOL).all()
    assert (np.abs(got["theta"] - lam[1:]) <= got["residual"] + n * dr.EPS).all()
    bound = sr.vector_bound(got["residual"], gap[1:], n)
    assert (np.linalg.norm(got["V"] - U[:, 1:], axis=0) <= bound).all()
    assert (sr.sign_margin(U[:, 1:]) > 2 * bound).all()              # so the sign rule picks the same component on both sides
    if name == "small":
        assert got["steps"] == n - 1 < dr.basis(k) and got["restarts"] == 0   # the Krylov space is exhausted before the basis is full


def test_emulation_restarts_at_least_twice_on_the_restart_case():
    name, n_comps = dr.RESTART_CASE
    got = dr.emulated(name, n_comps)
    assert got["restarts"] >= 2 and got["steps"] > dr.basis(n_comps - 1)


def test_gap_table():
    """the smallest gap among lambda_1 .. lambda_16 of the issue's three graphs, with and without density normalisation"""
    want = {("slab14", True): 2.4e-3, ("slab64", True): 5.3e-3, ("ribbon", True): 3.6e-3, ("slab14", False): 1.6e-3, ("slab64", False): 3.4e-3,
            ("ribbon", False): 1.4e-3}
    for (name, density), g in want.items():
        T, _ = dr.operator(*dr.case(name), density)
        w = np.linalg.eigvalsh(T)[::-1]
        got = np.diff(-w[:18])[1:17].min()
        print(name, density, got)
        assert abs(got - g) <= 0.05e-3 + 0.02 * g, (name, density, got)


def test_path_graph_does_not_converge_under_its_cap():
    got = dr.emulated("path", 16, True, dr.PATH_CAP)
    assert got["outcome"] == 2 and got["steps"] == dr.PATH_CAP and got["restarts"] >= 2 and got["residual"].max() > 1e-4 > dr.TOL
    T, _ = dr.operator(*dr.case("path"))
    assert 1.0 - np.linalg.eigvalsh(T)[-2] < 1e-5


def test_dpt_reference():
    T, q0, lam, U, gap = dr.dense("slab14", 16)
    d = dr.dpt(lam, U, [7, 400], n_dcs=10, normalize=False)
    assert d.shape == (1025, 2) and d[7, 0] == 0.0 and d[400, 1] == 0.0 and d[400, 0] == d[7, 1]
    w = lam[1:10] / (1 - lam[1:10])
    assert abs(d[33, 0] - np.sqrt((w ** 2 * (U[7, 1:10] - U[33, 1:10]) ** 2).sum())) <= 16 * dr.EPS * d[33, 0]
    dn = dr.dpt(lam, U, [7, 400], n_dcs=10, normalize=True)
    assert dn.max(0).tolist() == [1.0, 1.0]
    V = U.copy()
    V[5] = np.nan
    assert np.isinf(dr.dpt(lam, V, 7)[5, 0])


# ---- 4. the refusals before the library -----------------------------------------------------------------------------------------------
def test_python_refusals(sharp):
    rp, col, val = dr.case("small")
    for bad in (1, 65, 2.5):
        with pytest.raises(sharp.SharpError, match="n_comps must be an integer in 2 .. 64"):
            sharp.diffmap_graph(rp, col, val, n_comps=bad)
    for root in (20, 1000, -2):
        with pytest.raises(sharp.SharpError, match="root"):
            sharp.diffmap_graph(rp, col, val, n_comps=4, root=root)
    with pytest.raises(sharp.SharpError, match="not symmetric"):
        v2 = val.copy()
        v2[0] *= 2
        sharp.diffmap_graph(rp, col, v2, n_comps=4)
    with pytest.raises(sharp.SharpError, match="fewer than n_comps \\+ 2"):
        sharp.diffmap_graph(rp, col, val, n_comps=19)
    rpe, cole, vale = dr.with_empty_row(rp, col, val)
    with pytest.raises(sharp.SharpError, match="holds 1 row .* fewer than n_comps \\+ 2"):
        sharp.diffmap_graph(rpe, cole, vale, n_comps=4, root=5)
    with pytest.raises(sharp.SharpError, match="fewer than n_comps \\+ 2"):
        sharp.diffmap(np.zeros((5, 3)), n_neighbors=3, n_comps=4)
    with pytest.raises(sharp.SharpError, match="n_comps"):
        sharp.diffmap_neighbors(np.zeros((30, 3), np.int32), np.ones((30, 3)), n_comps=1)
    dm = {"evals": np.linspace(1.0, 0.5, 6), "evecs": np.ones((30, 6))}
    for bad in (1, 7, 10):
        with pytest.raises(sharp.SharpError, match="n_dcs must be an integer in 2 .. n_comps"):
            sharp.dpt(dm, root=0, n_dcs=bad)
    for root in (30, -1):
        with pytest.raises(sharp.SharpError, match="root out of range"):
            sharp.dpt(dm, root=root, n_dcs=4)
    with pytest.raises(sharp.SharpError, match="give root or roots"):
        sharp.dpt(dm, n_dcs=4)
    dm["evecs"][3] = np.nan
    with pytest.raises(sharp.SharpError, match="outside the component"):
        sharp.dpt(dm, root=3, n_dcs=4)


@pytest.mark.parametrize("name", ["diffmap", "diffmap_neighbors", "diffmap_graph", "dpt", "transitions", "component"])
def test_every_entry_reports_the_missing_device(sharp, monkeypatch, name):
    import torch

    from sharp_amd.diffmap import _component, _transitions

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rp, col, val = dr.case("small")
    idx = ((np.arange(40)[:, None] + np.arange(1, 4)[None, :]) % 40).astype(np.int32)
    calls = {
        "diffmap": lambda: sharp.diffmap(np.random.default_rng(0).normal(size=(40, 5)), n_neighbors=5, n_comps=4),
        "diffmap_neighbors": lambda: sharp.diffmap_neighbors(idx, np.ones((40, 3)), n_comps=4),
        "diffmap_graph": lambda: sharp.diffmap_graph(rp, col, val, n_comps=4, root=2),
        "dpt": lambda: sharp.dpt({"evals": np.linspace(1.0, 0.5, 4), "evecs": np.ones((20, 4))}, roots=[0, 3], n_dcs=3),
        "transitions": lambda: _transitions(rp, col, val),
        "component": lambda: _component(rp, col, val, 4),
    }
    monkeypatch.setattr(sharp._lib, "_initialised_device", 0)
    with pytest.raises(sharp.SharpError, match="no device context|no HIP device"):
        calls[name]()


# ---- 5. the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_typed(sharp):
    from sharp_amd import _abi

    L = sharp.lib()
    for name in ("sharp_diffmap_graph", "sharp_diffmap_neighbors", "sharp_diffmap_transitions", "sharp_diffmap_component", "sharp_dpt"):
        assert hasattr(L, name) and name in _abi.SIGNATURES
        twin = name.replace("sharp_", "sharp_C_", 1)
        assert hasattr(L, twin) and _abi.SIGNATURES[twin] == "v:" + "p" * (len(_abi.SIGNATURES[name]) - 2 + 1)
    assert _abi.SIGNATURES["sharp_dpt"] == "i:ppliipiip"
    assert sharp.diffmap is not None and sharp.dpt is not None


def test_dotc_twins_report_the_missing_device(sharp):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = sharp.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    I = lambda v: np.array([v], np.int32)                            # noqa: E731
    D = lambda v: np.array([v], np.float64)                          # noqa: E731
    rp, col, val = dr.case("small")
    rpd, n = rp.astype(np.float64), 20
    st = I(-1)
    L.sharp_C_diffmap_graph(*[P(v) for v in [rpd, col, val, D(n), I(4), I(1), D(-1), D(0.0), I(0), np.zeros(4), np.zeros((n, 4)), np.zeros(4),
                                            np.zeros(n, np.int32), I(0), I(0), D(0), D(0), I(0), st]])
    assert st[0] == 3                                                # SHARP_ERR_NO_DEVICE
    st[0] = -1
    L.sharp_C_diffmap_transitions(*[P(v) for v in [rpd, col, val, D(n), I(1), np.zeros(n), np.zeros(n), st]])
    assert st[0] == 3
    st[0] = -1
    L.sharp_C_diffmap_component(*[P(v) for v in [rpd, col, val, D(n), I(4), D(-1), I(0), D(0), D(0), D(0), np.zeros(n + 1), np.zeros(col.size, np.int32),
                                                np.zeros(col.size), np.zeros(n, np.int32), st]])
    assert st[0] == 3
    st[0] = -1
    L.sharp_C_dpt(*[P(v) for v in [np.linspace(1.0, 0.5, 4), np.ones((n, 4)), D(n), I(4), I(3), np.zeros(2, np.int32), I(2), I(1), np.zeros((n, 2)), st]])
    assert st[0] == 3 and b"no device context" in L.sharp_last_error()
