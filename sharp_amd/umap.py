"""uwot::umap on the MI355X, beside Rtsne: the map single-cell users reach for right after clustering.

uwot's argument names and defaults; the algorithm is this project's specification, modelled on umap-learn's and on
uwot's batch = TRUE mode -- no bit parity with either is claimed.  Computed by libsharp_hip.so (sharp_umap): the optional PCA and the
exact k-NN are Rtsne's own stages, the fuzzy graph and the epoch optimiser are HIP kernels, the a / b curve is fitted on the host.
umap_neighbors() takes neighbour lists the caller already has -- what knn() returns -- so lists computed once serve both maps.
umap_transform() places new rows in a fitted map: a UmapModel keeps the reference rows and their map on the device,
and every new row is placed by its nearest reference rows, block after block; knn_query() returns those lists alone.
There is no CPU path: without a device every call but umap_ab raises SharpError."""
import ctypes as C
import warnings
import weakref

import numpy as np

from . import _lib
from ._lib import check, f64, i32, i64, lib
from .tsne import _neighbour_arrays

__all__ = ["umap", "umap_neighbors", "umap_ab", "umap_transform", "UmapModel", "knn_query"]

_INITS = ("pca", "random")
_NORMLAPLACIAN = "normlaplacian"                 # init code 3; not an index into _INITS
_INIT_NAMES = {0: "pca", 1: "random", 2: "matrix", 3: _NORMLAPLACIAN}
_OUTCOMES = {0: "converged", 1: "not connected", 2: "not converged"}


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
        if init not in _INITS + (_NORMLAPLACIAN,):
            raise _lib.SharpError(f"{who}: init must be one of {_INITS + (_NORMLAPLACIAN,)} or an n x n_components matrix, not {init!r}")
        if init == "pca" and not allow_pca:
            raise _lib.SharpError(f"{who}: init = \"pca\" needs the data; give \"random\", \"normlaplacian\" or an n x n_components matrix")
        if init == _NORMLAPLACIAN and n < dims + 2:
            raise _lib.SharpError(f"{who}: init = \"normlaplacian\" needs at least n_components + 2 rows")
        code = 3 if init == _NORMLAPLACIAN else _INITS.index(init)
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


def _init_info(who):
    """sharp_umap_init_info of the call that just returned, as the result's "init"; a fallback is a RuntimeWarning"""
    req, used, steps, comp, res = C.c_int(), C.c_int(), C.c_int(), C.c_longlong(), C.c_double()
    check(lib().sharp_umap_init_info(C.byref(req), C.byref(used), C.byref(comp), C.byref(steps), C.byref(res)))
    info = {"requested": _INIT_NAMES[req.value], "used": _INIT_NAMES[used.value], "components": comp.value, "steps": steps.value,
            "residual": res.value}
    if used.value != req.value:
        why = (f"the graph has {comp.value} connected components" if comp.value != 1 else
               f"the eigensolver did not converge in {steps.value} steps (residual estimate {res.value:.3g})")
        warnings.warn(f"{who}: init = \"{info['requested']}\" fell back to \"{info['used']}\": {why}", RuntimeWarning, stacklevel=3)
    return info


def umap(X, n_neighbors=15, n_components=2, metric="euclidean", n_epochs=None, learning_rate=1.0, init="pca", spread=1.0, min_dist=0.01,
         set_op_mix_ratio=1.0, local_connectivity=1.0, bandwidth=1.0, repulsion_strength=1.0, negative_sample_rate=5, a=None, b=None,
         pca=None, pca_center=True, seed=10, ret_nn=False, n_threads=None, n_sgd_threads=0, verbose=False, batch=True, ret_model=False,
         nn_method="exact", nn_args=None):
    """umap(X, ...) with uwot's arguments and defaults; returns {"Y", "a", "b", "n_epochs", "n_neighbors", "N"} and, with ret_nn,
    "nn": {"index", "distance"} (the exact k-NN lists: n x (n_neighbors - 1), 0-based, Euclidean, self excluded); with ret_model,
    "model": a UmapModel of (X, Y) for umap_transform (n_neighbors up to 255; not together with pca).

    n_neighbors counts the point itself (2 .. 256, below n); n_components is 1, 2 or 3; n_epochs None: 500 up to 10 000 rows, else 200;
    init "pca" (the first n_components principal components of the prepared input), "random" (runif(-10, 10) from R's set.seed(seed)
    stream), "normlaplacian" (the bottom eigenvectors of the fuzzy graph's normalised Laplacian, uwot's noise-free spectral start,
    DESIGN.md §15: the result gains "init": {"requested", "used", "components", "steps", "residual"}, and a graph in pieces or a solve
    that does not converge falls back to "pca" with a RuntimeWarning) or a matrix, each coordinate then mapped onto [0, 10]; pca: None, or a number of components the input is reduced to first
    (centred when pca_center).  a, b: None fits them from (spread, min_dist).  Only metric = "euclidean" and set_op_mix_ratio =
    local_connectivity = bandwidth = 1 are built: anything else is refused.  n_threads, n_sgd_threads, verbose and batch are accepted
    and ignored (the update is always the batch form: every row moves at once from the epoch's old positions).  Input NA / NaN / Inf
    is refused.  Two calls with the same input and seed give bitwise-identical Y on the same GPU.

    nn_method="descent" (uwot's "nndescent" too): the lists come from knn_descent() (approximate; nn_args: its
    keywords) instead of the exact search.  The stages are composed here -- the PCA if asked for, knn_descent, umap_neighbors, the "pca"
    start computed from the data as a matrix -- so the map is bitwise umap_neighbors' on knn(X, n_neighbors - 1, method="descent");
    ret_nn returns the approximate lists (and "nn"["method"]), ret_model works as before."""
    who = "umap"
    from .tsne import _nn_method

    if _nn_method(nn_method, who) == "descent":
        return _umap_descent(X, n_neighbors, n_components, metric, n_epochs, learning_rate, init, spread, min_dist, set_op_mix_ratio,
                             local_connectivity, bandwidth, repulsion_strength, negative_sample_rate, a, b, pca, pca_center, seed, ret_nn,
                             ret_model, nn_args)
    if nn_args:
        raise _lib.SharpError(f"{who}: nn_args belong to nn_method = \"descent\"")
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
    if ret_model and pca:
        raise _lib.SharpError(f"{who}: ret_model is not built together with pca (the PCA's rotation is not kept, so new rows could not be "
                              "brought into the model's space): reduce the data first and give pca = None")
    if ret_model and n_neighbors > 255:
        raise _lib.SharpError(f"{who}: ret_model needs n_neighbors <= 255 (a model's lists hold n_neighbors reference rows)")
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
    if code == 3:
        out["init"] = _init_info(who)
    if ret_nn:
        out["nn"] = {"index": nn_i, "distance": nn_d}
    if ret_model:
        out["model"] = UmapModel(X, Y, n_neighbors, out["a"], out["b"], n_epochs)
    return out


def _umap_descent(X, n_neighbors, n_components, metric, n_epochs, learning_rate, init, spread, min_dist, set_op_mix_ratio,
                  local_connectivity, bandwidth, repulsion_strength, negative_sample_rate, a, b, pca, pca_center, seed, ret_nn, ret_model,
                  nn_args):
    """umap(nn_method="descent"): umap()'s checks, then prepare, knn_descent and umap_neighbors"""
    from .tsne import _prepare, knn_descent

    who = "umap"
    _refuse_unbuilt(who, metric, set_op_mix_ratio, local_connectivity, bandwidth)
    X = _rows(X, who)
    n, d = X.shape
    n_neighbors = int(n_neighbors)
    if not 2 <= n_neighbors <= 256:
        raise _lib.SharpError(f"{who}: n_neighbors must be in 2 .. 256")
    if n_neighbors >= n:
        raise _lib.SharpError(f"{who}: n_neighbors must be smaller than the number of rows")
    dims = _common(who, n, n_components, n_epochs, init, a, b, True)[0]
    pca = 0 if pca is None else int(pca)
    if pca < 0:
        raise _lib.SharpError(f"{who}: pca must be None or a positive number of components")
    if ret_model and pca:
        raise _lib.SharpError(f"{who}: ret_model is not built together with pca (the PCA's rotation is not kept, so new rows could not be "
                              "brought into the model's space): reduce the data first and give pca = None")
    if ret_model and n_neighbors > 255:
        raise _lib.SharpError(f"{who}: ret_model needs n_neighbors <= 255 (a model's lists hold n_neighbors reference rows)")
    pca_start = isinstance(init, str) and init == "pca"
    if pca_start and (min(pca, d) if pca else d) < dims:
        raise _lib.SharpError(f"{who}: init = \"pca\" needs at least n_components columns")
    xp = _prepare(X, pca=True, initial_dims=pca, pca_center=pca_center, pca_scale=False, normalize=False) if pca else X
    if pca_start:
        init = _prepare(xp, pca=True, initial_dims=dims, pca_center=True, pca_scale=False, normalize=False)
    idx, dist = knn_descent(xp, n_neighbors - 1, **dict(nn_args or {}, squared=False, ret_info=False))
    out = umap_neighbors(idx, dist, n_components=dims, n_epochs=n_epochs, learning_rate=learning_rate, init=init, spread=spread,
                         min_dist=min_dist, repulsion_strength=repulsion_strength, negative_sample_rate=negative_sample_rate, a=a, b=b,
                         seed=seed)
    if ret_nn:
        out["nn"] = {"index": idx, "distance": dist, "method": "descent"}
    if ret_model:
        out["model"] = UmapModel(X, out["Y"], n_neighbors, out["a"], out["b"], out["n_epochs"])
    return out


# ---- new rows in a fitted map -----------------------------------------------------------------------------------------
def _free_model(handle):
    if _lib._initialised_device is not None:     # (after shutdown() the library has freed it already)
        lib().sharp_umap_model_free(handle)


class UmapModel:
    """A fitted map on the device (sharp_umap_model_create): the reference rows X_ref (n_ref x d), their map Y_ref (n_ref x 1 .. 3),
    n_neighbors (1 .. 255, <= n_ref: the number of reference rows a new row is placed by), the curve's a and b, and the fit's n_epochs
    (a transform runs a third of them by default).  umap(..., ret_model=True) returns one.  close() frees it; it is a context manager
    and is freed when collected; shutdown() frees what is left.  X_ref and Y_ref must be finite."""

    def __init__(self, X_ref, Y_ref, n_neighbors, a, b, n_epochs):
        who = "UmapModel"
        X_ref = _rows(X_ref, who)
        Y_ref = np.ascontiguousarray(Y_ref, dtype=np.float64)
        n, d = X_ref.shape
        if Y_ref.ndim != 2 or Y_ref.shape[0] != n or Y_ref.shape[1] not in (1, 2, 3):
            raise _lib.SharpError(f"{who}: Y_ref must be an n_ref x (1, 2 or 3) matrix, not of shape {Y_ref.shape}")
        n_neighbors = int(n_neighbors)
        if not 1 <= n_neighbors <= 255:
            raise _lib.SharpError(f"{who}: n_neighbors must be in 1 .. 255")
        if n_neighbors > n:
            raise _lib.SharpError(f"{who}: n_neighbors must not exceed the number of reference rows")
        if not (a > 0 and b > 0 and np.isfinite(a) and np.isfinite(b)):
            raise _lib.SharpError(f"{who}: a and b must be positive")
        if int(n_epochs) < 0:
            raise _lib.SharpError(f"{who}: n_epochs must be >= 0")
        _lib.ensure_init()
        h = C.c_int(0)
        check(lib().sharp_umap_model_create(f64(X_ref), n, int(d), d, f64(Y_ref), int(Y_ref.shape[1]), n_neighbors, float(a), float(b),
                                            int(n_epochs), C.byref(h)))
        self.handle = h.value
        self.n_ref, self.d, self.dims = n, int(d), int(Y_ref.shape[1])
        self.n_neighbors, self.a, self.b, self.n_epochs = n_neighbors, float(a), float(b), int(n_epochs)
        self._finalizer = weakref.finalize(self, _free_model, self.handle)

    def close(self):
        if self._finalizer.detach():
            check(lib().sharp_umap_model_free(self.handle))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _queries(X_new, model, who):
    if not isinstance(model, UmapModel):
        raise _lib.SharpError(f"{who}: model must be a UmapModel (umap(..., ret_model=True)[\"model\"])")
    X_new = _rows(X_new, who)
    if X_new.shape[0] < 1 or X_new.shape[1] != model.d:
        raise _lib.SharpError(f"{who}: X_new must hold at least one row of the model's {model.d} columns, not shape {X_new.shape}")
    return X_new


def umap_transform(X_new, model, n_epochs=None, learning_rate=1.0, negative_sample_rate=5, repulsion_strength=1.0, seed=10, row_offset=0,
                   ret_nn=False):
    """umap_transform(X_new, model, ...): the rows of X_new placed in the model's map; returns {"Y", "n_epochs", "N"} and, with ret_nn,
    "nn": {"index", "distance"} (each row's model.n_neighbors nearest reference rows: 0-based, Euclidean, sorted by (distance, index)).

    Every row starts at the weighted mean of its neighbours' positions and is then moved for n_epochs epochs (None: a third of the
    fit's, rounded down; 0 returns the start) by the attraction of its neighbours and negative_sample_rate (0 .. 64) drawn reference
    rows per firing neighbour; the reference map does not move.  A row's result depends on that row, the model, the arguments and
    row_offset + its row number alone: a long table transformed block by block, with row_offset = the block's first row, gives the bits
    of one call.  Input NA / NaN / Inf is refused."""
    who = "umap_transform"
    X_new = _queries(X_new, model, who)
    n = X_new.shape[0]
    E = model.n_epochs // 3 if n_epochs is None else int(n_epochs)
    if E < 0:
        raise _lib.SharpError(f"{who}: n_epochs must be >= 0")
    if int(row_offset) < 0:
        raise _lib.SharpError(f"{who}: row_offset must be >= 0")
    if not 0 <= int(negative_sample_rate) <= 64:
        raise _lib.SharpError(f"{who}: negative_sample_rate must be in 0 .. 64")
    _lib.ensure_init()
    K = model.n_neighbors
    Y = np.zeros((n, model.dims))
    nn_i = np.zeros((n, K), np.int32) if ret_nn else None
    nn_d = np.zeros((n, K)) if ret_nn else None
    check(lib().sharp_umap_transform(model.handle, f64(X_new), n, model.d, E, float(learning_rate), int(negative_sample_rate),
                                     float(repulsion_strength), float(seed), int(row_offset), f64(Y), i32(nn_i), f64(nn_d)))
    out = {"Y": Y, "n_epochs": E, "N": n}
    if ret_nn:
        out["nn"] = {"index": nn_i, "distance": nn_d}
    return out


def knn_query(model_or_X_ref, X_new, K, max_rows_per_launch=0):
    """The K exact nearest rows of a reference for every row of X_new: (index (n_new, K) int32, 0-based into the reference; distance
    (n_new, K) Euclidean), ties to the lower index, each row sorted by (distance, index) -- a label transfer needs no more.  The
    reference is a UmapModel, or a matrix X_ref (a model is then made for the call and freed).  1 <= K <= 255, K <= n_ref.
    max_rows_per_launch (0: the library's choice) only cuts the work into launches; the lists do not depend on it."""
    who = "knn_query"
    K = int(K)
    if not 1 <= K <= 255:
        raise _lib.SharpError(f"{who}: K must be in 1 .. 255")
    if isinstance(model_or_X_ref, UmapModel):
        return _knn_cross(model_or_X_ref, X_new, K, max_rows_per_launch, who)
    X_ref = _rows(model_or_X_ref, who)
    if K > X_ref.shape[0]:
        raise _lib.SharpError(f"{who}: K must not exceed the number of reference rows")
    with UmapModel(X_ref, np.zeros((X_ref.shape[0], 1)), K, 1.0, 1.0, 0) as m:
        return _knn_cross(m, X_new, K, max_rows_per_launch, who)


def _knn_cross(model, X_new, K, max_rows_per_launch=0, who="knn_query"):
    """sharp_knn_cross"""
    X_new = _queries(X_new, model, who)
    if K > model.n_ref:
        raise _lib.SharpError(f"{who}: K must not exceed the number of reference rows")
    if int(max_rows_per_launch) < 0:
        raise _lib.SharpError(f"{who}: max_rows_per_launch must be >= 0")
    _lib.ensure_init()
    n = X_new.shape[0]
    idx = np.zeros((n, K), np.int32)
    dist = np.zeros((n, K))
    check(lib().sharp_knn_cross(model.handle, f64(X_new), n, model.d, int(K), int(max_rows_per_launch), i32(idx), f64(dist)))
    return idx, dist


def _transform_weights(model, index, distance):
    """(sigma, w, Y0) from a query's lists (sharp_umap_transform_weights)"""
    index = np.ascontiguousarray(index, np.int32)
    distance = np.ascontiguousarray(distance, np.float64)
    if index.ndim != 2 or index.shape != distance.shape:
        raise _lib.SharpError("umap_transform weights: index and distance must be matrices of one shape")
    n, K = index.shape
    _lib.ensure_init()
    sigma, w, Y0 = np.zeros(n), np.zeros((n, K)), np.zeros((n, model.dims))
    check(lib().sharp_umap_transform_weights(model.handle, i32(index), f64(distance), n, int(K), f64(sigma), f64(w), f64(Y0)))
    return sigma, w, Y0


def _transform_epochs(model, index, w, Y, n_epochs, ep0, ep1, learning_rate=1.0, negative_sample_rate=5, repulsion_strength=1.0, seed=10,
                      row_offset=0):
    """Y after epochs [ep0, ep1) of n_epochs from the given Y (sharp_umap_transform_epochs)"""
    index = np.ascontiguousarray(index, np.int32)
    w = np.ascontiguousarray(w, np.float64)
    Y = np.array(Y, dtype=np.float64, order="C")
    if index.ndim != 2 or index.shape != w.shape or Y.shape != (index.shape[0], model.dims):
        raise _lib.SharpError("umap_transform epochs: index and w must be matrices of one shape, Y nq x the model's dims")
    n, K = index.shape
    _lib.ensure_init()
    check(lib().sharp_umap_transform_epochs(model.handle, i32(index), f64(w), n, int(K), f64(Y), int(n_epochs), int(ep0), int(ep1),
                                            float(learning_rate), int(negative_sample_rate), float(repulsion_strength), float(seed),
                                            int(row_offset)))
    return Y


def umap_neighbors(index, distance, squared=False, n_components=2, n_epochs=None, learning_rate=1.0, init="random", spread=1.0,
                   min_dist=0.01, repulsion_strength=1.0, negative_sample_rate=5, a=None, b=None, seed=10, metric="euclidean",
                   set_op_mix_ratio=1.0, local_connectivity=1.0, bandwidth=1.0, n_threads=None, n_sgd_threads=0, verbose=False, batch=True):
    """umap_neighbors(index, distance, ...): the map from neighbour lists the caller already has -- what knn(X, K) returns: index
    (n x K, integers, 0-based), distance (n x K) their Euclidean distances, or their squares with squared=True.  n_neighbors is K + 1;
    1 <= K <= 255, K <= n - 1.  The lists are validated on the GPU as Rtsne_neighbors validates them.  init is "random", a matrix, or
    "normlaplacian" (as in umap(); it needs only the graph and falls back to "random" with a RuntimeWarning) -- there is no data for a
    PCA start.  With a given init, knn(X, K)'s lists give the bits of umap(X, n_neighbors=K + 1)."""
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
    out = {"Y": Y, "a": float(ab[0]), "b": float(ab[1]), "n_epochs": n_epochs, "n_neighbors": K + 1, "N": n}
    if code == 3:
        out["init"] = _init_info(who)
    return out


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


def _csr(row_ptr, col, val, who):
    rp = np.ascontiguousarray(row_ptr, np.int64)
    cc = np.ascontiguousarray(col, np.int32)
    if rp.ndim != 1 or rp.size < 2 or cc.ndim != 1 or rp[0] != 0 or rp[-1] != cc.size:
        raise _lib.SharpError(f"{who}: row_ptr must hold n + 1 values from 0 to the number of entries of col")
    vv = None
    if val is not None:
        vv = np.ascontiguousarray(val, np.float64)
        if vv.shape != cc.shape:
            raise _lib.SharpError(f"{who}: col and val must be vectors of one length")
    return rp, cc, vv


def _components(row_ptr, col):
    """(label, count) of a CSR pattern (sharp_umap_components): label[i] = the smallest vertex of i's connected component"""
    rp, cc, _ = _csr(row_ptr, col, None, "umap components")
    n = rp.size - 1
    _lib.ensure_init()
    label = np.zeros(n, np.int32)
    count = C.c_longlong()
    check(lib().sharp_umap_components(i64(rp), i32(cc) if cc.size else None, n, i32(label), C.byref(count)))
    return label, count.value


def _spectral(row_ptr, col, val, dims=2, tol=0.0, max_steps=0, V=None):
    """the spectral start's solve on a symmetric CSR (sharp_umap_spectral): {"V" (n x dims), "theta", "residual", "steps",
    "components", "outcome": 0 converged / 1 not connected / 2 not converged}.  tol, max_steps <= 0: the library's defaults.  V: an
    n x dims float64 buffer to fill (it is left as it is unless the outcome is 0)."""
    who = "umap spectral"
    rp, cc, vv = _csr(row_ptr, col, val, who)
    n = rp.size - 1
    dims = int(dims)
    if dims not in (1, 2, 3):
        raise _lib.SharpError(f"{who}: n_components must be 1, 2 or 3")
    if n < dims + 2:
        raise _lib.SharpError(f"{who}: needs at least n_components + 2 rows")
    if vv is None:
        raise _lib.SharpError(f"{who}: col and val must be vectors of one length")
    if V is None:
        V = np.zeros((n, dims))
    if not isinstance(V, np.ndarray) or V.dtype != np.float64 or V.shape != (n, dims) or not V.flags.c_contiguous:
        raise _lib.SharpError(f"{who}: V must be a C-contiguous float64 array of shape (n, n_components)")
    _lib.ensure_init()
    theta, residual = np.zeros(dims), np.zeros(dims)
    steps, outcome, comp = C.c_int(), C.c_int(), C.c_longlong()
    check(lib().sharp_umap_spectral(i64(rp), i32(cc) if cc.size else None, f64(vv), n, dims, float(tol), int(max_steps), f64(V), f64(theta),
                                    f64(residual), C.byref(steps), C.byref(comp), C.byref(outcome)))
    return {"V": V, "theta": theta, "residual": residual, "steps": steps.value, "components": comp.value, "outcome": outcome.value}


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
