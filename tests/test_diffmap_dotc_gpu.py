"""The .C() twins of the diffusion-map entries: sharp_C_diffmap_graph, sharp_C_diffmap_neighbors,
sharp_C_diffmap_transitions, sharp_C_diffmap_component and sharp_C_dpt give the bits of the C entries, and they turn refusals into *status with the message in
sharp_C_last_error -- what r/sharp_hip.R turns into stop()."""
import ctypes as C

import numpy as np
import pytest

import _diffmap_ref as dr
import _umap_spectral_ref as sr

pytestmark = pytest.mark.gpu

P = lambda a: a.ctypes.data_as(C.c_void_p)                           # noqa: E731
I = lambda v: np.array([v], np.int32)                                # noqa: E731
D = lambda v: np.array([v], np.float64)                              # noqa: E731


@pytest.fixture(scope="module")
def sharp():
    import sharp_amd

    sharp_amd.init(0)
    return sharp_amd


def _message(L):
    buf = C.create_string_buffer(b" " * 511)
    msg, ln = (C.c_char_p * 1)(C.addressof(buf)), (C.c_int * 1)(512)
    L.sharp_C_last_error(msg, ln)
    return buf.value


def _graph_twin(L, rp, col, val, n_comps, density=1, root=-1, tol=0.0, cap=0):
    n = rp.size - 1
    out = {"evals": np.zeros(n_comps), "evecs": np.zeros((n, n_comps)), "residual": np.zeros(n_comps), "in": np.zeros(n, np.int32),
           "steps": I(-1), "restarts": I(-1), "components": D(-1), "size": D(-1), "outcome": I(-1), "status": I(-1)}
    L.sharp_C_diffmap_graph(*[P(v) for v in [rp.astype(np.float64), col, val, D(n), I(n_comps), I(density), D(root), D(tol), I(cap), out["evals"],
                                            out["evecs"], out["residual"], out["in"], out["steps"], out["restarts"], out["components"],
                                            out["size"], out["outcome"], out["status"]]])
    return out


def test_graph_twin_gives_the_entrys_bits(sharp):
    import warnings

    L = sharp.lib()
    rp, col, val = dr.case("two_slabs")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want = sharp.diffmap_graph(rp, col, val, n_comps=6, root=3)
    got = _graph_twin(L, rp, col, val, 6, root=3)
    assert got["status"][0] == 0 and got["outcome"][0] == 0 and got["components"][0] == 2 and got["size"][0] == 512
    assert got["steps"][0] == want["steps"] and got["restarts"][0] == want["restarts"]
    assert np.array_equal(got["evecs"], want["evecs"], equal_nan=True) and np.array_equal(got["evals"], want["evals"])
    assert np.array_equal(got["residual"], want["residual"]) and np.array_equal(got["in"].astype(bool), want["in_component"])
    # refusals: the status and the message
    for kw, text in ((dict(n_comps=1), b"n_comps must be in 2 .. 64"), (dict(n_comps=6, root=5000), b"root must be -1 or a row"),
                     (dict(n_comps=6, tol=float("nan")), b"tol must be finite")):
        bad = _graph_twin(L, rp, col, val, **kw)
        assert bad["status"][0] == 2 and text in _message(L), kw
    bad = _graph_twin(L, *sr.edges_and_triangle(), 4)
    assert bad["status"][0] == 2 and b"holds 3 rows, fewer than n_comps + 2" in _message(L)
    assert bad["components"][0] == 513 and bad["size"][0] == 3


def test_neighbors_twin_gives_the_entrys_bits(sharp):
    L = sharp.lib()
    idx, d = sr.lists("ribbon", 14)
    d = np.ascontiguousarray(d)
    n = idx.shape[0]
    want = sharp.diffmap_neighbors(idx, d, n_comps=5)
    evals, evecs, res, inside = np.zeros(5), np.zeros((n, 5)), np.zeros(5), np.zeros(n, np.int32)
    steps, restarts, comps, size, outcome, st = I(-1), I(-1), D(-1), D(-1), I(-1), I(-1)
    L.sharp_C_diffmap_neighbors(*[P(v) for v in [idx, d, D(n), I(14), I(0), I(5), I(1), D(-1), D(0.0), I(0), evals, evecs, res, inside, steps,
                                                restarts, comps, size, outcome, st]])
    assert st[0] == 0 and outcome[0] == 0 and comps[0] == 1 and size[0] == n and steps[0] == want["steps"] and inside.all()
    assert np.array_equal(evecs, want["evecs"]) and np.array_equal(evals, want["evals"]) and np.array_equal(res, want["residual"])
    L.sharp_C_diffmap_neighbors(*[P(v) for v in [idx, d, D(n), I(14), I(0), I(70), I(1), D(-1), D(0.0), I(0), evals, evecs, res, inside, steps,
                                                restarts, comps, size, outcome, st]])
    assert st[0] == 2 and b"n_comps must be in 2 .. 64" in _message(L)


def test_stage_twins_give_the_entries_bits(sharp):
    from sharp_amd.diffmap import _component, _transitions

    L = sharp.lib()
    rp, col, val = dr.case("two_slabs")
    n = rp.size - 1
    rpd, st = rp.astype(np.float64), I(-1)
    for density in (1, 0):
        a, z = np.zeros(n), np.zeros(n)
        L.sharp_C_diffmap_transitions(*[P(v) for v in [rpd, col, val, D(n), I(density), a, z, st]])
        wa, wz = _transitions(rp, col, val, bool(density))
        assert st[0] == 0 and np.array_equal(a, wa) and np.array_equal(z, wz)
    label, comps, sn, snnz = I(-1), D(-1), D(-1), D(-1)
    srp, scol, sval, new_id = np.zeros(n + 1), np.zeros(col.size, np.int32), np.zeros(col.size), np.zeros(n, np.int32)
    L.sharp_C_diffmap_component(*[P(v) for v in [rpd, col, val, D(n), I(4), D(-1), label, comps, sn, snnz, srp, scol, sval, new_id, st]])
    want = _component(rp, col, val, 4)
    assert st[0] == 0 and label[0] == want[0] == 512 and comps[0] == want[1] == 2 and sn[0] == 513 and snnz[0] == want[2][1].size
    assert np.array_equal(srp[:514], want[2][0].astype(np.float64)) and np.array_equal(scol[:int(snnz[0])], want[2][1])
    assert np.array_equal(sval[:int(snnz[0])], want[2][2]) and np.array_equal(new_id, want[3])
    L.sharp_C_diffmap_component(*[P(v) for v in [rpd, col, val, D(n), I(4), D(n), label, comps, sn, snnz, srp, scol, sval, new_id, st]])
    assert st[0] == 2 and b"root must be -1 or a row" in _message(L)
    bad = col.copy()
    bad[7] = n
    L.sharp_C_diffmap_transitions(*[P(v) for v in [rpd, bad, val, D(n), I(1), np.zeros(n), np.zeros(n), st]])
    assert st[0] == 2 and b"column index out of range" in _message(L)


def test_dpt_twin_gives_the_entrys_bits(sharp):
    L = sharp.lib()
    T, q0, lam, U, gap = dr.dense("ribbon", 8)
    n = U.shape[0]
    V = np.ascontiguousarray(U)
    roots = np.array([0, 100, 256], np.int32)
    for normalize in (1, 0):
        out, st = np.zeros((n, 3)), I(-1)
        L.sharp_C_dpt(*[P(v) for v in [lam, V, D(n), I(8), I(6), roots, I(3), I(normalize), out, st]])
        assert st[0] == 0 and np.array_equal(out, sharp.dpt({"evals": lam, "evecs": V}, roots=roots, n_dcs=6, normalize=bool(normalize)))
    out, st = np.zeros((n, 3)), I(-1)
    L.sharp_C_dpt(*[P(v) for v in [lam, V, D(n), I(8), I(9), roots, I(3), I(1), out, st]])
    assert st[0] == 2 and b"n_dcs must be in 2 .. n_comps" in _message(L)
    L.sharp_C_dpt(*[P(v) for v in [lam, V, D(n), I(8), I(6), np.array([0, n, 5], np.int32), I(3), I(1), out, st]])
    assert st[0] == 2 and b"a root out of range" in _message(L)
