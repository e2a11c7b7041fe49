"""Rtsne on the MI355X: the 2-D map that visualization_SHARP draws (R/visualization_SHARP.R:94 calls Rtsne there).

Rtsne's interface and defaults, bhtsne's algorithm, computed by libsharp_hip.so (sharp_tsne):
PCA / normalisation, exact k-NN, per-row perplexity calibration and the optimiser loop all run as HIP kernels.
There is no CPU path: without a device every call raises SharpError."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib

__all__ = ["Rtsne"]


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _rows(X):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("Rtsne: X must be a matrix")
    return np.ascontiguousarray(X)


def _n_itercosts(max_iter):
    return sum(1 for it in range(max_iter) if (it > 0 and it % 50 == 0) or it == max_iter - 1)


_REPULSIONS = ("exact", "barnes_hut")


def _check_repulsion(repulsion):
    if repulsion not in _REPULSIONS:
        raise _lib.SharpError(f"Rtsne: repulsion must be one of {_REPULSIONS}, not {repulsion!r}")


def Rtsne(X, dims=2, initial_dims=50, perplexity=30, theta=0.5, check_duplicates=True, pca=True, partial_pca=False, max_iter=1000,
          verbose=False, is_distance=False, Y_init=None, pca_center=True, pca_scale=False, normalize=True, stop_lying_iter=None,
          mom_switch_iter=None, momentum=0.5, final_momentum=0.8, eta=200.0, exaggeration_factor=12.0, num_threads=1, seed=10,
          repulsion="exact"):
    """Rtsne(X, ...) with Rtsne's arguments and defaults; returns Rtsne's list as a dict
    (Y, itercosts, costs, N, origD, perplexity, theta, max_iter, ...).

    repulsion="exact" (the default): the repulsion is computed EXACTLY -- the theta -> 0 limit of Barnes-Hut -- so `theta` is accepted
    for compatibility and unused.  The cost is O(n^2) per iteration (measured on one MI355X, 2-D: 1.16 ms per iteration at 50 000
    points, 81 ms at 500 000; README).
    repulsion="barnes_hut": bhtsne's Barnes-Hut repulsion, theta honoured as Rtsne does (0 <= theta <= 1, else "Incorrect theta.";
    theta = 0 is the exact path bit for bit): a quadtree (octree in 3-D, binary tree in 1-D) of Y rebuilt on the GPU at every
    iteration, O(n log n) work per iteration (DESIGN.md §10 "Barnes-Hut"; README has the measured times).
    Either way the input similarities come from the floor(3 perplexity) exact nearest neighbours (perplexity <= 85), an exact k-NN of
    O(n^2 d).  Without Y_init the start is 1e-4 N(0, 1) drawn from R's set.seed(seed) stream (polar method); two calls with the same
    input and seed give bitwise-identical Y on the same GPU.  num_threads, verbose and partial_pca are accepted and ignored;
    is_distance is not supported."""
    _check_repulsion(repulsion)
    if is_distance:
        raise _lib.SharpError("Rtsne: is_distance = TRUE is not supported")
    X = _rows(X)
    n, d = X.shape
    dims = int(dims)
    if dims not in (1, 2, 3):
        raise _lib.SharpError("Rtsne: dims must be 1, 2 or 3")
    if Y_init is not None:
        Y_init = np.ascontiguousarray(Y_init, dtype=np.float64)
        if Y_init.shape != (n, dims):
            raise _lib.SharpError("Rtsne: Y_init must be an n x dims matrix")
    if stop_lying_iter is None:
        stop_lying_iter = 0 if Y_init is not None else 250
    if mom_switch_iter is None:
        mom_switch_iter = 0 if Y_init is not None else 250
    _lib.ensure_init()
    Y = np.zeros((n, dims))
    ic = np.zeros(max(1, _n_itercosts(int(max_iter))))
    costs = np.zeros(n)
    entry = lib().sharp_tsne_bh if repulsion == "barnes_hut" else lib().sharp_tsne
    check(entry(_dp(X), C.c_longlong(n), int(d), C.c_longlong(d), dims, int(initial_dims), int(bool(pca)), int(bool(pca_center)),
                           int(bool(pca_scale)), int(bool(normalize)), int(bool(check_duplicates)), C.c_double(perplexity), C.c_double(theta),
                           int(max_iter), int(stop_lying_iter), int(mom_switch_iter), C.c_double(momentum), C.c_double(final_momentum),
                           C.c_double(eta), C.c_double(exaggeration_factor), _dp(Y_init), C.c_double(seed), _dp(Y), _dp(ic), _dp(costs)))
    return {"Y": Y, "itercosts": ic[: _n_itercosts(int(max_iter))], "costs": costs, "N": n,
            "origD": min(int(initial_dims), d) if pca else d, "perplexity": perplexity, "theta": theta, "max_iter": int(max_iter),
            "stop_lying_iter": int(stop_lying_iter), "mom_switch_iter": int(mom_switch_iter), "momentum": momentum,
            "final_momentum": final_momentum, "eta": eta, "exaggeration_factor": exaggeration_factor, "pca": bool(pca),
            "normalize": bool(normalize)}


# ---- the stages one at a time (tests, tools/bench_tsne.py) ----------------------------------------------------------------------------
def _prepare(X, pca=True, initial_dims=50, pca_center=True, pca_scale=False, normalize=True):
    X = _rows(X)
    n, d = X.shape
    _lib.ensure_init()
    out = np.zeros((n, d))
    dd = C.c_int()
    check(lib().sharp_tsne_prepare(_dp(X), C.c_longlong(n), d, C.c_longlong(d), int(pca), int(initial_dims), int(pca_center),
                                   int(pca_scale), int(normalize), _dp(out), C.byref(dd)))
    return np.ascontiguousarray(out.reshape(-1)[: n * dd.value].reshape(n, dd.value))


def _knn(X, K):
    X = _rows(X)
    n, d = X.shape
    _lib.ensure_init()
    idx = np.zeros((n, K), np.int32)
    dist = np.zeros((n, K))
    check(lib().sharp_tsne_knn(_dp(X), C.c_longlong(n), d, C.c_longlong(d), int(K), idx.ctypes.data_as(C.POINTER(C.c_int)), _dp(dist)))
    return idx, dist


def _affinities(X, perplexity):
    """P (CSR: row_ptr, col, val) of the already prepared X"""
    X = _rows(X)
    n, d = X.shape
    _lib.ensure_init()
    cap = 2 * n * int(np.floor(3 * perplexity))
    rp = np.zeros(n + 1, np.int64)
    col = np.zeros(max(cap, 1), np.int32)
    val = np.zeros(max(cap, 1))
    nnz = C.c_longlong()
    check(lib().sharp_tsne_affinities(_dp(X), C.c_longlong(n), d, C.c_longlong(d), C.c_double(perplexity), C.c_longlong(cap),
                                      rp.ctypes.data_as(C.POINTER(C.c_longlong)), col.ctypes.data_as(C.POINTER(C.c_int)), _dp(val), C.byref(nnz)))
    return rp, col[: nnz.value].copy(), val[: nnz.value].copy()


def _gradient(row_ptr, col, val, Y):
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    n, dims = Y.shape
    _lib.ensure_init()
    rp = np.ascontiguousarray(row_ptr, np.int64)
    cc = np.ascontiguousarray(col, np.int32)
    vv = np.ascontiguousarray(val, np.float64)
    dY = np.zeros_like(Y)
    check(lib().sharp_tsne_gradient(rp.ctypes.data_as(C.POINTER(C.c_longlong)), cc.ctypes.data_as(C.POINTER(C.c_int)), _dp(vv),
                                    C.c_longlong(n), dims, _dp(Y), _dp(dY)))
    return dY


def _gradient_bh(row_ptr, col, val, Y, theta=0.5):
    """the gradient with the Barnes-Hut repulsion at theta, and the Z it used: (dY, Z)"""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    n, dims = Y.shape
    _lib.ensure_init()
    rp = np.ascontiguousarray(row_ptr, np.int64)
    cc = np.ascontiguousarray(col, np.int32)
    vv = np.ascontiguousarray(val, np.float64)
    dY = np.zeros_like(Y)
    Z = C.c_double()
    check(lib().sharp_tsne_gradient_bh(rp.ctypes.data_as(C.POINTER(C.c_longlong)), cc.ctypes.data_as(C.POINTER(C.c_int)), _dp(vv),
                                       C.c_longlong(n), dims, _dp(Y), C.c_double(theta), _dp(dY), C.byref(Z)))
    return dY, Z.value
