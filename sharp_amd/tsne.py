"""Rtsne on the MI355X: the 2-D map that visualization_SHARP draws (R/visualization_SHARP.R:94 calls Rtsne there).

Rtsne's interface and defaults, bhtsne's algorithm, computed by libsharp_hip.so (sharp_tsne):
PCA / normalisation, exact k-NN, per-row perplexity calibration and the optimiser loop all run as HIP kernels.
Rtsne's two other ways in are here too: Rtsne(d, is_distance=True) on a dist vector or a square matrix (sharp_tsne_dist) and
Rtsne_neighbors(index, distance) on neighbour lists the caller already has (sharp_tsne_neighbors), with knn() to compute such lists
once and reuse them for every later map of the same data.
There is no CPU path: without a device every call raises SharpError."""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, f64, i32, i64, lib

__all__ = ["Rtsne", "Rtsne_neighbors", "knn", "knn_descent"]


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


def _condensed(X, who):
    """R's dist vector (n (n - 1) / 2 doubles) and n from a dist vector or a square matrix; a matrix must equal its transpose exactly
    and is condensed on the host, its diagonal ignored.  Entries must be finite and >= 0.  No device is touched."""
    a = np.asarray(X, dtype=np.float64)
    if a.ndim == 1:
        n = (1 + math.isqrt(1 + 8 * a.size)) // 2
        if n < 2 or n * (n - 1) // 2 != a.size:
            raise _lib.SharpError(f"{who}: a dist vector holds n (n - 1) / 2 entries; {a.size} is no such length")
        d = np.ascontiguousarray(a)
    elif a.ndim == 2 and a.shape[0] == a.shape[1] and a.shape[0] >= 2:
        n = a.shape[0]
        if not np.array_equal(a, a.T, equal_nan=True):
            raise _lib.SharpError(f"{who}: the distance matrix is not symmetric (it must equal its transpose exactly)")
        d = np.concatenate([a[i, i + 1:] for i in range(n)])          # row-wise upper triangle = column-wise lower triangle
    else:
        raise _lib.SharpError(f"{who}: with is_distance, X must be a dist vector or a square matrix")
    if not (d >= 0).all() or not np.isfinite(d).all():                # (NaN fails the first test)
        raise _lib.SharpError(f"{who}: the distances hold NA / NaN / Inf or a negative value")
    if n > 46340:
        raise _lib.SharpError(f"{who}: more than 46340 objects (the dist vector would pass 2^30 entries) is not supported")
    return d, n


def _loop_args(n, dims, Y_init, stop_lying_iter, mom_switch_iter, who):
    dims = int(dims)
    if dims not in (1, 2, 3):
        raise _lib.SharpError(f"{who}: dims must be 1, 2 or 3")
    if Y_init is not None:
        Y_init = np.ascontiguousarray(Y_init, dtype=np.float64)
        if Y_init.shape != (n, dims):
            raise _lib.SharpError(f"{who}: Y_init must be an n x dims matrix")
    if stop_lying_iter is None:
        stop_lying_iter = 0 if Y_init is not None else 250
    if mom_switch_iter is None:
        mom_switch_iter = 0 if Y_init is not None else 250
    return dims, Y_init, int(stop_lying_iter), int(mom_switch_iter)


def _optimise(entry, head, n, dims, origD, pca, normalize, perplexity, theta, max_iter, stop_lying_iter, mom_switch_iter, momentum,
              final_momentum, eta, exaggeration_factor, Y_init, seed):
    """One run of an optimiser entry (sharp_tsne / sharp_tsne_bh, sharp_tsne_dist, sharp_tsne_neighbors) -> Rtsne's list.  head: the
    entry's own leading arguments, up to where all of them go on alike: perplexity .. seed, then the outputs Y, itercosts, costs."""
    _lib.ensure_init()
    Y = np.zeros((n, dims))
    ic = np.zeros(max(1, _n_itercosts(int(max_iter))))
    costs = np.zeros(n)
    check(entry(*head, perplexity, theta, int(max_iter), stop_lying_iter, mom_switch_iter, momentum, final_momentum, eta, exaggeration_factor,
                f64(Y_init), seed, f64(Y), f64(ic), f64(costs)))
    return {"Y": Y, "itercosts": ic[: _n_itercosts(int(max_iter))], "costs": costs, "N": n, "origD": origD, "perplexity": perplexity,
            "theta": theta, "max_iter": int(max_iter), "stop_lying_iter": stop_lying_iter, "mom_switch_iter": mom_switch_iter,
            "momentum": momentum, "final_momentum": final_momentum, "eta": eta, "exaggeration_factor": exaggeration_factor,
            "pca": bool(pca), "normalize": bool(normalize)}


def Rtsne(X, dims=2, initial_dims=50, perplexity=30, theta=0.5, check_duplicates=True, pca=True, partial_pca=False, max_iter=1000,
          verbose=False, is_distance=False, Y_init=None, pca_center=True, pca_scale=False, normalize=True, stop_lying_iter=None,
          mom_switch_iter=None, momentum=0.5, final_momentum=0.8, eta=200.0, exaggeration_factor=12.0, num_threads=1, seed=10,
          repulsion="exact", nn_method="exact", nn_args=None):
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
    input and seed give bitwise-identical Y on the same GPU.  num_threads, verbose and partial_pca are accepted and ignored.

    is_distance=True: X is a dist vector of length n (n - 1) / 2 (what sharp_amd.dist returns) or an n x n matrix, n <= 46340.  A matrix
    must equal its transpose exactly; its diagonal is ignored.  Every distance must be finite and >= 0.  The floor(3 perplexity)
    nearest objects of each are selected on the distances as given (ties to the lower index) and P is built from their squares.
    pca, initial_dims, normalize and check_duplicates are ignored for a distance input, and origD is None.

    nn_method="descent" ("nndescent"): the neighbours come from knn_descent() (approximate; nn_args: its keywords) instead
    of the exact search.  The stages are composed here -- prepare, knn_descent, Rtsne_neighbors -- so the map is bitwise what
    Rtsne_neighbors gives on knn(prepared X, floor(3 perplexity), squared=True, method="descent"); check_duplicates then looks at each
    row's nearest kept neighbour.  Not together with is_distance."""
    _check_repulsion(repulsion)
    if _nn_method(nn_method, "Rtsne") == "descent":
        if is_distance:
            raise _lib.SharpError("Rtsne: nn_method = \"descent\" needs the rows of X; it is not built together with is_distance")
        if not (np.isfinite(perplexity) and perplexity > 0):
            raise _lib.SharpError("Rtsne: perplexity must be positive")
        if perplexity > 85:
            raise _lib.SharpError("Rtsne: perplexity above 85 is not supported (at most 255 neighbours per row)")
        X = _rows(X)
        if X.shape[0] - 1 < 3 * perplexity:
            raise _lib.SharpError("Perplexity is too large.")
        xp = _prepare(X, pca=pca, initial_dims=initial_dims, pca_center=pca_center, pca_scale=pca_scale, normalize=normalize)
        idx, d2 = knn_descent(xp, int(np.floor(3 * perplexity)), squared=True, **dict(nn_args or {}, ret_info=False))
        if check_duplicates and (d2[:, 0] == 0).any():
            raise _lib.SharpError("Remove duplicates before running TSNE.")
        out = Rtsne_neighbors(idx, d2, dims=dims, perplexity=perplexity, theta=theta, max_iter=max_iter, Y_init=Y_init,
                              stop_lying_iter=stop_lying_iter, mom_switch_iter=mom_switch_iter, momentum=momentum,
                              final_momentum=final_momentum, eta=eta, exaggeration_factor=exaggeration_factor, seed=seed,
                              repulsion=repulsion, squared=True)
        out.update(origD=min(int(initial_dims), X.shape[1]) if pca else X.shape[1], pca=bool(pca), normalize=bool(normalize))
        return out
    if nn_args:
        raise _lib.SharpError("Rtsne: nn_args belong to nn_method = \"descent\"")
    if is_distance:
        d, n = _condensed(X, "Rtsne")
    else:
        X = _rows(X)
        n, d = X.shape
    dims, Y_init, stop_lying_iter, mom_switch_iter = _loop_args(n, dims, Y_init, stop_lying_iter, mom_switch_iter, "Rtsne")
    loop = (perplexity, theta, max_iter, stop_lying_iter, mom_switch_iter, momentum, final_momentum, eta, exaggeration_factor, Y_init, seed)
    if is_distance:
        return _optimise(lib().sharp_tsne_dist, (f64(d), int(n), int(repulsion == "barnes_hut"), dims), n, dims, None, False, False, *loop)
    head = (f64(X), n, int(d), d, dims, int(initial_dims), int(bool(pca)), int(bool(pca_center)), int(bool(pca_scale)), int(bool(normalize)),
            int(bool(check_duplicates)))
    return _optimise(lib().sharp_tsne_bh if repulsion == "barnes_hut" else lib().sharp_tsne, head, n, dims,
                     min(int(initial_dims), d) if pca else d, pca, normalize, *loop)


def _neighbour_arrays(index, distance, who):
    """(index int32, distance float64), both n x K and C-contiguous; refusals that need no device"""
    index = np.asarray(index)
    distance = np.asarray(distance)
    if index.ndim != 2 or distance.ndim != 2:
        raise _lib.SharpError(f"{who}: index and distance must be n x K matrices")
    if index.shape != distance.shape:
        raise _lib.SharpError(f"{who}: index {index.shape} and distance {distance.shape} differ in shape")
    if not np.issubdtype(index.dtype, np.integer):
        raise _lib.SharpError(f"{who}: index must hold integers, not {index.dtype}")
    if not (np.issubdtype(distance.dtype, np.floating) or np.issubdtype(distance.dtype, np.integer)):
        raise _lib.SharpError(f"{who}: distance must hold real numbers, not {distance.dtype}")
    n, K = index.shape
    if n < 2:
        raise _lib.SharpError(f"{who}: need at least 2 rows")
    if K < 1:
        raise _lib.SharpError(f"{who}: need at least one neighbour per row (K >= 1)")
    if K > 255:
        raise _lib.SharpError(f"{who}: at most 255 neighbours per row")
    if K > n - 1:
        raise _lib.SharpError(f"{who}: K neighbours per row need K <= n - 1")
    if index.dtype != np.int32:
        # an index that int32 cannot hold is out of range whatever n is: keep it so (the library names its row)
        index = np.where((index < -1) | (index > 2 ** 31 - 1), -1, index)
    return np.ascontiguousarray(index, np.int32), np.ascontiguousarray(distance, np.float64)


def Rtsne_neighbors(index, distance, dims=2, perplexity=30, theta=0.5, max_iter=1000, Y_init=None, stop_lying_iter=None,
                    mom_switch_iter=None, momentum=0.5, final_momentum=0.8, eta=200.0, exaggeration_factor=12.0, num_threads=1, seed=10,
                    repulsion="exact", squared=False):
    """Rtsne_neighbors(index, distance, ...): the map from neighbour lists the caller already has.  index (n x K, integers, 0-based)
    names each row's K neighbours and distance (n x K) their Euclidean distances, or their squares with squared=True -- what
    knn(X, K, squared=True) returns.  1 <= K <= 255, K <= n - 1, perplexity <= K (the entropy of K neighbours cannot pass log K) and
    n - 1 >= 3 perplexity.  The lists are validated on the GPU before use (every index in [0, n), no row naming itself, no index twice
    in a row, distances finite and >= 0) and used in the caller's order: knn()'s lists give the bits of
    Rtsne(X, pca=False, normalize=False, check_duplicates=False).  Everything else is Rtsne's; origD is None."""
    who = "Rtsne_neighbors"
    _check_repulsion(repulsion)
    index, distance = _neighbour_arrays(index, distance, who)
    n, K = index.shape
    dims, Y_init, stop_lying_iter, mom_switch_iter = _loop_args(n, dims, Y_init, stop_lying_iter, mom_switch_iter, who)
    head = (i32(index), f64(distance), n, int(K), int(bool(squared)), int(repulsion == "barnes_hut"), dims)
    return _optimise(lib().sharp_tsne_neighbors, head, n, dims, None, False, False, perplexity, theta, max_iter, stop_lying_iter,
                     mom_switch_iter, momentum, final_momentum, eta, exaggeration_factor, Y_init, seed)


_NN_METHODS = {"exact": "exact", "descent": "descent", "nndescent": "descent"}      # ("nndescent": uwot's spelling)


def _nn_method(nn_method, who):
    if nn_method not in _NN_METHODS:
        raise _lib.SharpError(f"{who}: nn_method must be \"exact\" or \"descent\" (\"nndescent\"), not {nn_method!r}")
    return _NN_METHODS[nn_method]


def knn_descent(X, K, squared=False, n_projections=8, max_candidates=None, n_iters=12, delta=0.001, seed=10, ret_info=False):
    """The approximate K nearest neighbours of every row by NN-descent on the GPU (sharp_knn_descent), in knn()'s format:
    (index (n, K) int32, 0-based; distance (n, K)), self excluded, no index twice, each row sorted by (distance, index).  Every pair a list
    keeps carries bitwise the distance knn() gives that pair; what is approximate is which rows a list holds.  The start offers each row
    the K rows on either side of it in each of n_projections (1 .. 32) sorted random projections; then at most n_iters joins over
    max_candidates (1 .. 255; None: min(K, 30)) sampled reverse neighbours, until a join changes <= delta n K entries.  The lists are a
    pure function of the arguments (seed: a whole number in [0, 2^53)): two calls give the same bits.  With K = n - 1 they are the exact
    lists.  ret_info=True adds {"joins", "updates", "reason": "n_iters" / "delta", "gathered" (the candidate rows the joins measured),
    "method": "descent"}.  1 <= K <= 255, K <= n - 1."""
    who = "knn_descent"
    X = _rows(X)
    K = int(K)
    n, d = X.shape
    if not 1 <= K <= 255:
        raise _lib.SharpError(f"{who}: K must be in 1 .. 255")
    if K > n - 1:
        raise _lib.SharpError(f"{who}: K neighbours per row need K <= n - 1")
    if not 1 <= int(n_projections) <= 32:
        raise _lib.SharpError(f"{who}: n_projections must be in 1 .. 32")
    S = 0 if max_candidates is None else int(max_candidates)
    if max_candidates is not None and not 1 <= S <= 255:
        raise _lib.SharpError(f"{who}: max_candidates must be in 1 .. 255 (None: min(K, 30))")
    if int(n_iters) < 0:
        raise _lib.SharpError(f"{who}: n_iters must be >= 0")
    if not 0 <= float(delta) <= 1:                                    # (false for NaN too)
        raise _lib.SharpError(f"{who}: delta must be in [0, 1]")
    _lib.ensure_init()
    idx = np.zeros((n, K), np.int32)
    d2 = np.zeros((n, K))
    info = np.zeros(4, np.int64)
    check(lib().sharp_knn_descent(f64(X), n, int(d), d, K, int(n_projections), S, int(n_iters), float(delta), float(seed), i32(idx), f64(d2),
                                  i64(info)))
    out = (idx, d2) if squared else (idx, np.sqrt(d2))
    if ret_info:
        return out + ({"joins": int(info[0]), "updates": int(info[1]), "reason": ("n_iters", "delta")[int(info[2])], "gathered": int(info[3]),
                       "method": "descent"},)
    return out


def knn(X, K, squared=False, is_distance=False, method="exact", **descent_args):
    """The K nearest neighbours of every row: (index (n, K) int32, 0-based; distance (n, K)), self excluded, ties to the lower
    index, each row sorted by (distance, index).  From the rows of X (the k-NN Rtsne itself runs; Euclidean distances, or their squares
    sum (x_i - x_j)^2 with squared=True), or with is_distance=True from a dist vector or a square matrix as Rtsne(is_distance=True)
    takes it: then the selection is on the distances as given, and they are returned as given (squared=True: their squares).
    1 <= K <= 255, K <= n - 1.  The lists suit every perplexity <= K / 3 of Rtsne_neighbors.
    method="exact" (the default): the exact lists, O(n^2 d).  method="descent" ("nndescent"): knn_descent()'s approximate lists in the
    same format, its arguments as keywords (n_projections, max_candidates, n_iters, delta, seed); not together with is_distance."""
    K = int(K)
    if _nn_method(method, "knn") == "descent":
        if is_distance:
            raise _lib.SharpError("knn: method = \"descent\" needs the rows of X; it is not built together with is_distance")
        descent_args.pop("ret_info", None)
        return knn_descent(X, K, squared=squared, **descent_args)
    if descent_args:
        raise _lib.SharpError(f"knn: {sorted(descent_args)} belong to method = \"descent\"")
    if is_distance:
        d, n = _condensed(X, "knn")
        if not 1 <= K <= min(255, n - 1):
            raise _lib.SharpError("knn: need 1 <= K <= 255 and K <= n - 1")
        _lib.ensure_init()
        idx = np.zeros((n, K), np.int32)
        d2 = np.zeros((n, K))
        check(lib().sharp_tsne_knn_dist(f64(d), int(n), K, i32(idx), f64(d2)))
        if squared:
            return idx, d2
        # the distances as given, not a root of their squares: entry (i, j) of the dist vector (i < j) sits at n i - i (i + 1) / 2 + j - i - 1
        i = np.minimum(np.arange(n, dtype=np.int64)[:, None], idx)
        j = np.maximum(np.arange(n, dtype=np.int64)[:, None], idx)
        return idx, d[n * i - i * (i + 1) // 2 + j - i - 1]
    X = _rows(X)
    if not 1 <= K <= min(255, X.shape[0] - 1):
        raise _lib.SharpError("knn: need 1 <= K <= 255 and K <= n - 1")
    idx, d2 = _knn(X, K)
    return (idx, d2) if squared else (idx, np.sqrt(d2))


# ---- the stages one at a time (tests, tools/bench_tsne.py) ----------------------------------------------------------------------------
def _prepare(X, pca=True, initial_dims=50, pca_center=True, pca_scale=False, normalize=True):
    X = _rows(X)
    n, d = X.shape
    _lib.ensure_init()
    out = np.zeros((n, d))
    dd = C.c_int()
    check(lib().sharp_tsne_prepare(f64(X), n, d, d, int(pca), int(initial_dims), int(pca_center), int(pca_scale), int(normalize), f64(out),
                                   C.byref(dd)))
    return np.ascontiguousarray(out.reshape(-1)[: n * dd.value].reshape(n, dd.value))


def _knn(X, K):
    X = _rows(X)
    n, d = X.shape
    _lib.ensure_init()
    idx = np.zeros((n, K), np.int32)
    dist = np.zeros((n, K))
    check(lib().sharp_tsne_knn(f64(X), n, d, d, int(K), i32(idx), f64(dist)))
    return idx, dist


def _knn_descent_start(X, K, n_projections=8, seed=10, max_rows_per_launch=0):
    """knn_descent's start alone (sharp_knn_descent_start): (index, squared distance)"""
    X = _rows(X)
    n, d = X.shape
    _lib.ensure_init()
    idx = np.zeros((n, int(K)), np.int32)
    d2 = np.zeros((n, int(K)))
    check(lib().sharp_knn_descent_start(f64(X), n, int(d), d, int(K), int(n_projections), float(seed), int(max_rows_per_launch), i32(idx),
                                        f64(d2)))
    return idx, d2


def _knn_descent_join(X, index, max_candidates=None, iteration=1, seed=10, max_rows_per_launch=0):
    """one join from given lists (sharp_knn_descent_join): (index, squared distance, entries that changed)"""
    X = _rows(X)
    n, d = X.shape
    index = np.ascontiguousarray(index, np.int32)
    if index.ndim != 2 or index.shape[0] != n:
        raise _lib.SharpError("knn_descent join: index must be an n x K matrix")
    K = index.shape[1]
    _lib.ensure_init()
    idx = np.zeros((n, K), np.int32)
    d2 = np.zeros((n, K))
    upd = C.c_longlong()
    check(lib().sharp_knn_descent_join(f64(X), n, int(d), d, int(K), i32(index), 0 if max_candidates is None else int(max_candidates),
                                       int(iteration), float(seed), int(max_rows_per_launch), i32(idx), f64(d2), C.byref(upd)))
    return idx, d2, upd.value


def _affinities_nn(index, distance, perplexity, squared=False):
    """P (CSR: row_ptr, col, val) from given neighbour lists (sharp_tsne_affinities_nn)"""
    index, distance = _neighbour_arrays(index, distance, "affinities")
    n, K = index.shape
    _lib.ensure_init()
    cap = 2 * n * K
    rp = np.zeros(n + 1, np.int64)
    col = np.zeros(cap, np.int32)
    val = np.zeros(cap)
    nnz = C.c_longlong()
    check(lib().sharp_tsne_affinities_nn(i32(index), f64(distance), n, int(K), int(bool(squared)), perplexity, cap, i64(rp), i32(col),
                                         f64(val), C.byref(nnz)))
    return rp, col[: nnz.value].copy(), val[: nnz.value].copy()


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
    check(lib().sharp_tsne_affinities(f64(X), n, d, d, perplexity, cap, i64(rp), i32(col), f64(val), C.byref(nnz)))
    return rp, col[: nnz.value].copy(), val[: nnz.value].copy()


def _gradient(row_ptr, col, val, Y):
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    n, dims = Y.shape
    _lib.ensure_init()
    rp = np.ascontiguousarray(row_ptr, np.int64)
    cc = np.ascontiguousarray(col, np.int32)
    vv = np.ascontiguousarray(val, np.float64)
    dY = np.zeros_like(Y)
    check(lib().sharp_tsne_gradient(i64(rp), i32(cc), f64(vv), n, dims, f64(Y), f64(dY)))
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
    check(lib().sharp_tsne_gradient_bh(i64(rp), i32(cc), f64(vv), n, dims, f64(Y), theta, f64(dY), C.byref(Z)))
    return dY, Z.value
