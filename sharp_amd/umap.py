"""uwot::umap on the MI355X, beside Rtsne: the map single-cell users reach for right after clustering.

uwot's argument names and defaults; the algorithm is this project's specification, modelled on umap-learn's and on
uwot's batch = TRUE mode -- no bit parity with either is claimed.  Computed by libsharp_hip.so (sharp_umap): the optional PCA and the
exact k-NN are Rtsne's own stages, the fuzzy graph and the epoch optimiser are HIP kernels, the a / b curve is fitted on the host.
umap_neighbors() takes neighbour lists the caller already has -- what knn() returns -- so lists computed once serve both maps.
There is no CPU path: without a device every call but umap_ab raises SharpError."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, f64, i32, i64, lib
from .tsne import _neighbour_arrays

__all__ = ["umap", "umap_neighbors", "umap_ab"]

_INITS = ("pca", "random")


def _rows(X, who):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise _lib.SharpError(f"{who}: X must be a matrix")
    return np.ascontiguousarray(X)


def umap_ab(spread=1.0, min_dist=0.01):
    """(a, b) of the curve 1 / (1 + a x^(2b)) fitted to y = 1 below min_dist, exp(-(x - min_dist) / spread) above, on the 300 points
    linspace(0, 3 spread): a host Levenberg-Marquardt in the library (sharp_umap_ab); needs no device."""
    a, b = C.c_double(), C.c_double()
    check(lib().sharp_umap_ab(float(spread), float(min_dist), C.byref(a), C.byref(b)))
    return a.value, b.value


def _refuse_unbuilt(who, metric, set_op_mix_ratio, local_connectivity, bandwidth):
    if metric != "euclidean":
        raise _lib.SharpError(f"{who}: metric {metric!r} is not supported (only \"euclidean\")")
    for name, v in (("set_op_mix_ratio", set_op_mix_ratio), ("local_connectivity", local_connectivity), ("bandwidth", bandwidth)):
        if v != 1:
            raise _lib.SharpError(f"{who}: {name} = {v!r} is not supported (only 1)")


def _common(who, n, n_components, n_epochs, init, a, b, allow_pca):
    """the checks that need no device -> (dims, n_epochs, init code, Y_init, ab)"""
    dims = int(n_components)
    if dims not in (1, 2, 3):
        raise _lib.SharpError(f"{who}: n_components must be 1, 2 or 3")
    if n_epochs is None:
        n_epochs = 500 if n <= 10000 else 200
    n_epochs = int(n_epochs)
    if n_epochs < 0:
        raise _lib.SharpError(f"{who}: n_epochs must be >= 0")
    Y_init = None
    if isinstance(init, str):
        if init not in _INITS:
            raise _lib.SharpError(f"{who}: init must be one of {_INITS} or an n x n_components matrix, not {init!r}")
        if init == "pca" and not allow_pca:
            raise _lib.SharpError(f"{who}: init = \"pca\" needs the data; give \"random\" or an n x n_components matrix")
        code = _INITS.index(init)
    else:
        Y_init = np.ascontiguousarray(init, dtype=np.float64)
        if Y_init.shape != (n, dims):
            raise _lib.SharpError(f"{who}: init must be \"pca\", \"random\" or an n x n_components matrix, not a matrix of shape {Y_init.shape}")
        code = 2
    if (a is None) != (b is None):
        raise _lib.SharpError(f"{who}: give both a and b, or neither")
    if a is not None and not (a > 0 and b > 0 and np.isfinite(a) and np.isfinite(b)):
        raise _lib.SharpError(f"{who}: a and b must be positive")
    ab = np.array([0.0, 0.0] if a is None else [float(a), float(b)])
    return dims, n_epochs, code, Y_init, ab


def umap(X, n_neighbors=15, n_components=2, metric="euclidean", n_epochs=None, learning_rate=1.0, init="pca", spread=1.0, min_dist=0.01,
         set_op_mix_ratio=1.0, local_connectivity=1.0, bandwidth=1.0, repulsion_strength=1.0, negative_sample_rate=5, a=None, b=None,
         pca=None, pca_center=True, seed=10, ret_nn=False, n_threads=None, n_sgd_threads=0, verbose=False, batch=True):
    """umap(X, ...) with uwot's arguments and defaults; returns {"Y", "a", "b", "n_epochs", "n_neighbors", "N"} and, with ret_nn,
    "nn": {"index", "distance"} (the exact k-NN lists: n x (n_neighbors - 1), 0-based, Euclidean, self excluded).

    n_neighbors counts the point itself (2 .. 256, below n); n_components is 1, 2 or 3; n_epochs None: 500 up to 10 000 rows, else 200;
    init "pca" (the first n_components principal components of the prepared input), "random" (runif(-10, 10) from R's set.seed(seed)
    stream) or a matrix, each coordinate then mapped onto [0, 10]; pca: None, or a number of components the input is reduced to first
    (centred when pca_center).  a, b: None fits them from (spread, min_dist).  Only metric = "euclidean" and set_op_mix_ratio =
    local_connectivity = bandwidth = 1 are built: anything else is refused.  n_threads, n_sgd_threads, verbose and batch are accepted
    and ignored (the update is always the batch form: every row moves at once from the epoch's old positions).  Input NA / NaN / Inf
    is refused.  Two calls with the same input and seed give bitwise-identical Y on the same GPU."""
    who = "umap"
    _refuse_unbuilt(who, metric, set_op_mix_ratio, local_connectivity, bandwidth)
    X = _rows(X, who)
    n, d = X.shape
    n_neighbors = int(n_neighbors)
    if not 2 <= n_neighbors <= 256:
        raise _lib.SharpError(f"{who}: n_neighbors must be in 2 .. 256")
    if n_neighbors >= n:
        raise _lib.SharpError(f"{who}: n_neighbors must be smaller than the number of rows")
    dims, n_epochs, code, Y_init, ab = _common(who, n, n_components, n_epochs, init, a, b, True)
    pca = 0 if pca is None else int(pca)
    if pca < 0:
        raise _lib.SharpError(f"{who}: pca must be None or a positive number of components")
    if code == 0 and (min(pca, d) if pca else d) < dims:
        raise _lib.SharpError(f"{who}: init = \"pca\" needs at least n_components columns")
    _lib.ensure_init()
    K = n_neighbors - 1
    Y = np.zeros((n, dims))
    nn_i = np.zeros((n, K), np.int32) if ret_nn else None
    nn_d = np.zeros((n, K)) if ret_nn else None
    check(lib().sharp_umap(f64(X), n, int(d), d, n_neighbors, dims, n_epochs, float(learning_rate), float(min_dist), float(spread), f64(ab),
                           int(negative_sample_rate), float(repulsion_strength), code, f64(Y_init), pca, int(bool(pca_center)), float(seed),
                           f64(Y), i32(nn_i), f64(nn_d)))
    out = {"Y": Y, "a": float(ab[0]), "b": float(ab[1]), "n_epochs": n_epochs, "n_neighbors": n_neighbors, "N": n}
    if ret_nn:
        out["nn"] = {"index": nn_i, "distance": nn_d}
    return out


def umap_neighbors(index, distance, squared=False, n_components=2, n_epochs=None, learning_rate=1.0, init="random", spread=1.0,
                   min_dist=0.01, repulsion_strength=1.0, negative_sample_rate=5, a=None, b=None, seed=10, metric="euclidean",
                   set_op_mix_ratio=1.0, local_connectivity=1.0, bandwidth=1.0, n_threads=None, n_sgd_threads=0, verbose=False, batch=True):
    """umap_neighbors(index, distance, ...): the map from neighbour lists the caller already has -- what knn(X, K) returns: index
    (n x K, integers, 0-based), distance (n x K) their Euclidean distances, or their squares with squared=True.  n_neighbors is K + 1;
    1 <= K <= 255, K <= n - 1.  The lists are validated on the GPU as Rtsne_neighbors validates them.  init is "random" or a matrix
    (there is no data for a PCA start).  With a given init, knn(X, K)'s lists give the bits of umap(X, n_neighbors=K + 1)."""
    who = "umap_neighbors"
    _refuse_unbuilt(who, metric, set_op_mix_ratio, local_connectivity, bandwidth)
    index, distance = _neighbour_arrays(index, distance, who)
    n, K = index.shape
    dims, n_epochs, code, Y_init, ab = _common(who, n, n_components, n_epochs, init, a, b, False)
    _lib.ensure_init()
    Y = np.zeros((n, dims))
    check(lib().sharp_umap_neighbors(i32(index), f64(distance), n, int(K), int(bool(squared)), dims, n_epochs, float(learning_rate),
                                     float(min_dist), float(spread), f64(ab), int(negative_sample_rate), float(repulsion_strength), code,
                                     f64(Y_init), float(seed), f64(Y)))
    return {"Y": Y, "a": float(ab[0]), "b": float(ab[1]), "n_epochs": n_epochs, "n_neighbors": K + 1, "N": n}


# ---- the stages one at a time (tests, tools/bench_umap.py) ----------------------------------------------------------------------------
def _graph(index, distance, squared=False):
    """the fuzzy graph from neighbour lists (sharp_umap_graph): (row_ptr, col, val, rho, sigma)"""
    index, distance = _neighbour_arrays(index, distance, "umap graph")
    n, K = index.shape
    _lib.ensure_init()
    cap = 2 * n * K
    rp = np.zeros(n + 1, np.int64)
    col = np.zeros(cap, np.int32)
    val = np.zeros(cap)
    rho, sigma = np.zeros(n), np.zeros(n)
    nnz = C.c_longlong()
    check(lib().sharp_umap_graph(i32(index), f64(distance), n, int(K), int(bool(squared)), cap, i64(rp), i32(col), f64(val), C.byref(nnz),
                                 f64(rho), f64(sigma)))
    return rp, col[: nnz.value].copy(), val[: nnz.value].copy(), rho, sigma


def _epochs(row_ptr, col, val, Y, n_epochs, ep0, ep1, a, b, learning_rate=1.0, negative_sample_rate=5, repulsion_strength=1.0, seed=10):
    """Y after epochs [ep0, ep1) of n_epochs from the given Y (sharp_umap_epochs)"""
    Y = np.array(Y, dtype=np.float64, order="C")
    n, dims = Y.shape
    _lib.ensure_init()
    rp = np.ascontiguousarray(row_ptr, np.int64)
    cc = np.ascontiguousarray(col, np.int32)
    vv = np.ascontiguousarray(val, np.float64)
    check(lib().sharp_umap_epochs(i64(rp), i32(cc), f64(vv), n, dims, f64(Y), int(n_epochs), int(ep0), int(ep1), float(learning_rate),
                                  float(a), float(b), int(negative_sample_rate), float(repulsion_strength), float(seed)))
    return Y
