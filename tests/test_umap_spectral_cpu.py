"""UMAP's spectral start without a GPU: the premises of the numpy reference that the GPU tests compare against
(tests/_umap_spectral_ref.py), asserted so that the reference alone stays within every condition those comparisons rely on; the checks
of init = "normlaplacian" that happen before the library; and the new entries' export."""
import ctypes as C

import numpy as np
import pytest

import _umap_spectral_ref as sr


@pytest.fixture(scope="module")
def sharp():
    import os

    import __graft_entry__ as g

    import sharp_amd

    if not os.path.exists(sharp_amd.so_path()):
        g.build()
    return sharp_amd


# ---- 1. premises of the reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sr.SOLVER_CASES)
def test_solver_inputs_are_connected_separated_and_converge(name):
    rp, col, val = sr.case(name)
    n = rp.size - 1
    assert n == (257 if name == "ribbon" else 1025) and n % 64 != 0 and n % 256 != 0
    label, count = sr.components(rp, col)
    assert count == 1 and (label == 0).all()
    assert np.diff(rp).max() == {"hub": 688}.get(name, np.diff(rp).max())
    M, q0, lam, U, gap = sr.dense(name)
    assert np.abs(M - M.T).max() == 0.0                              # W's mirrored entries carry the same bits, and so do M's
    assert np.linalg.norm(M @ q0 - q0) <= 64 * sr.EPS                # q0 is the eigenvector of the eigenvalue 1
    assert (gap >= 1e-3).all(), gap
    got = sr.lanczos(M, q0, 3)
    assert got["outcome"] == 0 and got["steps"] <= sr.MAX_STEPS
    bound = sr.vector_bound(got["residual"], gap, n)
    print(f"{name}: theta {lam}, gaps {gap}, steps {got['steps']}, residuals {got['residual']}, vector bounds {bound}, sign margins "
          f"{sr.sign_margin(U)}")
    assert (got["residual"] <= sr.TOL).all()
    assert (sr.sign_margin(U) > 2 * bound).all()                     # so the sign rule picks the same component on both sides
    assert (np.abs(got["theta"] - lam) <= got["residual"] + n * sr.EPS).all()
    assert (np.linalg.norm(got["V"] - U, axis=0) <= bound).all()


def test_hub_row_needs_several_passes():
    rp, col, val = sr.case("hub")
    assert rp[1] - rp[0] == 688 > 10 * 64 and (val[rp[0]:rp[1]] == 0.25).sum() >= 600
    assert np.diff(sr.case("slab14")[0]).max() < 64 < np.diff(sr.case("slab64")[0]).max()


def test_inputs_of_the_other_outcomes():
    for name, want in (("two_slabs", 2), ("blobs", 6)):
        rp, col, _ = sr.case(name)
        label, count = sr.components(rp, col)
        assert count == want and np.unique(label).size == want
    rp, col, _ = sr.edges_and_triangle()
    assert rp.size - 1 == 1027 and sr.components(rp, col)[1] == 513
    rp, col, val = sr.case("path")
    assert sr.components(rp, col)[1] == 1 and np.diff(rp).max() == 2
    M, q0 = sr.operator(rp, col, val)
    got = sr.lanczos(M, q0, 3, max_steps=40)
    assert got["outcome"] == 2 and got["steps"] == 40 and got["residual"].max() > 1e-3 > sr.TOL


def test_start_vector_is_the_hash():
    x = sr.start_vector(5)
    assert x[0] == float(int(sr.ref.mix(np.uint64(sr.ref.GOLDEN))) >> 11) * 2.0 ** -53 - 0.5
    assert (np.abs(sr.start_vector(1025)) <= 0.5).all() and np.unique(sr.start_vector(1025)).size == 1025


# ---- 2. the checks before the library -------------------------------------------------------------------------------------------------
def _small():
    X = np.random.default_rng(0).normal(size=(40, 5))
    idx = ((np.arange(40)[:, None] + np.arange(1, 4)[None, :]) % 40).astype(np.int32)
    nd = np.random.default_rng(1).uniform(0.5, 2.0, size=(40, 3))
    return X, idx, nd


def test_other_spectral_names_are_still_refused(sharp):
    X, idx, nd = _small()
    for name in ("spectral", "laplacian", "agspectral", "NormLaplacian"):
        with pytest.raises(sharp.SharpError, match="init must be one of"):
            sharp.umap(X, init=name)
        with pytest.raises(sharp.SharpError, match="init must be one of"):
            sharp.umap_neighbors(idx, nd, init=name)
    with pytest.raises(sharp.SharpError, match="n_components \\+ 2 rows"):
        sharp.umap(np.zeros((4, 5)), n_neighbors=2, n_components=3, init="normlaplacian")


def _entries(s):
    from sharp_amd.umap import _components, _spectral

    X, idx, nd = _small()
    rp = np.arange(41, dtype=np.int64)
    col = ((np.arange(40) + 1) % 40).astype(np.int32)
    return {
        "umap": lambda: s.umap(X, n_neighbors=5, init="normlaplacian"),
        "umap_neighbors": lambda: s.umap_neighbors(idx, nd, init="normlaplacian"),
        "visualization_SHARP": lambda: s.visualization_SHARP({"x0": X, "viE": X}, method="umap", plot=False, n_neighbors=5,
                                                             init="normlaplacian"),
        "components": lambda: _components(rp, col),
        "spectral": lambda: _spectral(rp, col, np.ones(40), 2, 1e-8, 30),
    }


@pytest.mark.parametrize("name", ["umap", "umap_neighbors", "visualization_SHARP", "components", "spectral"])
def test_normlaplacian_enters_the_library(sharp, monkeypatch, name):
    """as tests/test_umap_cpu.py::test_every_entry_reports_the_missing_device: the Python checks pass, the arguments are converted and the
    library, which has no context here, answers with its own SharpError"""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    monkeypatch.setattr(sharp._lib, "_initialised_device", 0)
    with pytest.raises(sharp.SharpError, match="no device context|no HIP device"):
        _entries(sharp)[name]()


def test_spectral_wrapper_refusals(sharp):
    from sharp_amd.umap import _components, _spectral

    rp = np.arange(41, dtype=np.int64)
    col = ((np.arange(40) + 1) % 40).astype(np.int32)
    val = np.ones(40)
    for dims in (0, 4):
        with pytest.raises(sharp.SharpError, match="n_components must be 1, 2 or 3"):
            _spectral(rp, col, val, dims)
    with pytest.raises(sharp.SharpError, match="n_components \\+ 2 rows"):
        _spectral(rp[:5], col[:4] % 4, val[:4], 3)
    with pytest.raises(sharp.SharpError, match="one length"):
        _spectral(rp, col, val[:39], 2)
    with pytest.raises(sharp.SharpError, match="row_ptr must hold"):
        _spectral(rp[:40], col, val, 2)
    with pytest.raises(sharp.SharpError, match="row_ptr must hold"):
        _spectral(rp + 1, col, val, 2)
    with pytest.raises(sharp.SharpError, match="row_ptr must hold"):
        _components(rp.reshape(1, 41), col)
    for V in (np.zeros((40, 3)), np.zeros((40, 2), np.float32), np.zeros((2, 40)).T):
        with pytest.raises(sharp.SharpError, match="V must be a C-contiguous float64 array"):
            _spectral(rp, col, val, 2, V=V)


# ---- 3. the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_typed(sharp):
    from sharp_amd import _abi

    L = sharp.lib()
    for name in ("sharp_umap_components", "sharp_umap_spectral", "sharp_umap_init_info", "sharp_C_umap_components", "sharp_C_umap_spectral",
                 "sharp_C_umap_init_info"):
        assert hasattr(L, name) and name in _abi.SIGNATURES
    assert _abi.SIGNATURES["sharp_umap_spectral"] == "i:ppplidipppppp"


def test_dotc_twins_report_the_missing_device(sharp):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = sharp.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)                       # noqa: E731
    I = lambda v: np.array([v], np.int32)                            # noqa: E731
    D = lambda v: np.array([v], np.float64)                          # noqa: E731
    rp = np.arange(41, dtype=np.float64)
    col = ((np.arange(40) + 1) % 40).astype(np.int32)
    st = I(-1)
    L.sharp_C_umap_components(*[P(v) for v in [rp, col, D(40), np.zeros(40, np.int32), D(0), st]])
    assert st[0] == 3                                                # SHARP_ERR_NO_DEVICE
    st[0] = -1
    L.sharp_C_umap_spectral(*[P(v) for v in [rp, col, np.ones(40), D(40), I(2), D(0.0), I(0), np.zeros((40, 2)), np.zeros(2), np.zeros(2), I(0),
                                            D(0), I(0), st]])
    assert st[0] == 3
    st[0] = -1
    L.sharp_C_umap_init_info(*[P(v) for v in [I(0), I(0), D(0), I(0), D(0), st]])
    assert st[0] == 3 and b"no device context" in L.sharp_last_error()
