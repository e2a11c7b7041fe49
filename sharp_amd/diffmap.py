"""diffmap(), diffmap_neighbors(), diffmap_graph() and dpt(): a diffusion map of the neighbour graph and the diffusion pseudotime of
every cell from chosen root cells -- in scanpy's terms tl.diffmap and tl.dpt without the branchings.

The graph is the fuzzy union umap() builds from the k-NN lists -- scanpy's connectivities --, or any symmetric CSR the caller has, the
SNN graph included.  With q_i = sum_j W_ij and density_normalize (the default, scanpy's) K = Q^-1 W Q^-1, z_i = sum_j K_ij and
T = Z^-1/2 K Z^-1/2; without it K = W, z = q.  The map is made of the n_comps largest eigenpairs of the symmetric T: evals[0] = 1 with
evecs[:, 0] = sqrt(z) / ||sqrt(z)||, then the largest eigenvalues below it with their unit eigenvectors as they are (each vector's
largest |component| positive).  The solve runs on ONE connected component: the root's when a root is given, otherwise the largest (ties
to the component with the smallest vertex); cells outside it get NaN coordinates and an infinite pseudotime, and a RuntimeWarning
counts them.  The eigenpairs come from a thick-restart Lanczos in fp64 whose sums all run in a fixed order: two calls give the same
bits.  This is the project's own specification; no parity with scanpy or destiny is claimed.
Computed by libsharp_hip.so (csrc/diffmap.hip); there is no CPU path."""
import ctypes as C
import warnings

import numpy as np

from . import _lib
from ._lib import SharpError, check, f64, i32, i64, lib
from .community import _symmetric_csr
from .snn import _search
from .tsne import _neighbour_arrays

__all__ = ["diffmap", "diffmap_neighbors", "diffmap_graph", "dpt"]

MAX_COMPS = 64


def _limits(who, n_comps, tol, max_matvecs, root, n=None):
    """the refusals of the arguments that need no device -> (n_comps, tol, max_matvecs, root)"""
    if isinstance(n_comps, bool) or int(n_comps) != n_comps or not 2 <= int(n_comps) <= MAX_COMPS:
        raise SharpError(f"{who}: n_comps must be an integer in 2 .. {MAX_COMPS}")
    tol = float(tol)
    if not np.isfinite(tol):
        raise SharpError(f"{who}: tol must be finite (<= 0: the default, 1e-6)")
    if int(max_matvecs) != max_matvecs or not 0 <= int(max_matvecs) <= 10 ** 8:
        raise SharpError(f"{who}: max_matvecs must be an integer in 0 .. 1e8 (0: the default, 4000)")
    root = -1 if root is None else root
    if isinstance(root, (bool, float)) or int(root) != root or int(root) < -1:
        raise SharpError(f"{who}: root must be None or the 0-based number of a row")
    if n is not None:
        _size(who, n, int(n_comps), int(root))
    return int(n_comps), tol, int(max_matvecs), int(root)


def _size(who, n, n_comps, root):
    if root >= n:
        raise SharpError(f"{who}: root {root} is out of range (the graph has {n} rows, counted from 0)")
    if n < n_comps + 2:
        raise SharpError(f"{who}: the component holds at most {n} rows, fewer than n_comps + 2 = {n_comps + 2}")


class _Out:
    """the output buffers of a sharp_diffmap_* call, and the result dict and the warnings made of them"""

    def __init__(self, n, n_comps):
        self.n = n
        self.evals, self.evecs, self.residual = np.zeros(n_comps), np.zeros((n, n_comps)), np.zeros(n_comps)
        self.inside = np.zeros(n, np.int32)
        self.steps, self.restarts, self.outcome = C.c_int(), C.c_int(), C.c_int()
        self.comps, self.size = C.c_longlong(), C.c_longlong()

    def args(self):
        return (f64(self.evals), f64(self.evecs), f64(self.residual), i32(self.inside), C.byref(self.steps), C.byref(self.restarts),
                C.byref(self.comps), C.byref(self.size), C.byref(self.outcome))

    def result(self, who, density_normalize):
        comps, size = self.comps.value, self.size.value
        if comps > 1:
            warnings.warn(f"{who}: the graph has {comps} connected components; the one of {size} cells was solved and "
                          f"{self.n - size} cells are left out (NaN coordinates, infinite pseudotime)", RuntimeWarning, stacklevel=3)
        if self.outcome.value != 0:
            warnings.warn(f"{who}: not converged after {self.steps.value} operator applications: the largest residual is "
                          f"{self.residual.max():.3e}", RuntimeWarning, stacklevel=3)
        return {"evals": self.evals, "evecs": self.evecs, "residual": self.residual, "converged": self.outcome.value == 0,
                "steps": self.steps.value, "restarts": self.restarts.value, "components": comps, "component_size": size,
                "in_component": self.inside.astype(bool), "density_normalize": bool(density_normalize)}


def diffmap_graph(row_ptr, col, val, n_comps=15, density_normalize=True, root=None, tol=0.0, max_matvecs=0):
    """The diffusion map of any symmetric weighted graph given as a CSR (louvain_graph's input and refusals: col ascending within a row,
    no diagonal entry, val[i, j] == val[j, i] bit for bit).  Returns {"evals" (n_comps; evals[0] == 1.0), "evecs" (n x n_comps; NaN in the
    rows outside the solved component), "residual" (n_comps: the true ||T v - theta v|| of every returned vector), "converged" (every
    residual <= tol), "steps" (operator applications), "restarts", "components", "component_size", "in_component" (n, bool),
    "density_normalize"}.  2 <= n_comps <= 64; the solved component needs n_comps + 2 rows.  root: a 0-based row whose component is
    solved (None: the largest).  tol <= 0: 1e-6; max_matvecs 0: 4000.  Where the cap is reached the last Ritz vectors are still returned,
    with their residuals, converged False and a RuntimeWarning."""
    who = "diffmap_graph"
    rp, cc, vv = _symmetric_csr(row_ptr, col, val, who)
    n = rp.size - 1
    n_comps, tol, max_matvecs, root = _limits(who, n_comps, tol, max_matvecs, root, n)
    if root >= 0 and rp[root] == rp[root + 1]:
        raise SharpError(f"{who}: the component holds 1 row (root {root} has no neighbour), fewer than n_comps + 2 = {n_comps + 2}")
    _lib.ensure_init()
    o = _Out(n, n_comps)
    check(lib().sharp_diffmap_graph(i64(rp), i32(cc), f64(vv), n, n_comps, int(bool(density_normalize)), root, tol, max_matvecs, *o.args()))
    return o.result(who, density_normalize)


def diffmap_neighbors(index, distance, squared=False, n_comps=15, density_normalize=True, root=None, tol=0.0, max_matvecs=0):
    """The diffusion map of the fuzzy graph of neighbour lists the caller already has -- what knn(X, K) returns: index (n x K, 0-based),
    distance (n x K) Euclidean, or their squares with squared=True.  The graph is umap_neighbors' (n_neighbors = K + 1).  The result
    is built on the device and never leaves it; the result is diffmap_graph's on that graph, bit for bit."""
    who = "diffmap_neighbors"
    index, distance = _neighbour_arrays(index, distance, who)
    n, K = index.shape
    n_comps, tol, max_matvecs, root = _limits(who, n_comps, tol, max_matvecs, root, n)
    _lib.ensure_init()
    o = _Out(n, n_comps)
    check(lib().sharp_diffmap_neighbors(i32(index), f64(distance), n, int(K), int(bool(squared)), n_comps, int(bool(density_normalize)), root,
                                        tol, max_matvecs, *o.args()))
    return o.result(who, density_normalize)


def diffmap(X, n_neighbors=15, n_comps=15, nn_method="exact", nn_args=None, pca=None, pca_center=True, density_normalize=True, root=None,
            tol=0.0, max_matvecs=0, ret_nn=False):
    """The diffusion map of the neighbour graph of the rows of X, as sc.tl.diffmap computes it from scanpy's connectivities.  The input
    is prepared and searched as umap() does it: pca None or a number of components (centred when pca_center), n_neighbors counts the
    row itself (2 .. 256, below n), nn_method "exact" or "descent" (knn_descent()'s approximate lists, nn_args its keywords).  The
    result is diffmap_neighbors' on those lists; with ret_nn it also carries "nn": {"index", "distance"}."""
    who = "diffmap"
    from .tsne import _rows

    X = _rows(X)
    _limits(who, n_comps, tol, max_matvecs, root, X.shape[0] if X.ndim == 2 else None)
    idx, dist, method = _search(X, n_neighbors, nn_method, nn_args, pca, pca_center, who)
    out = diffmap_neighbors(idx, dist, False, n_comps, density_normalize, root, tol, max_matvecs)
    if ret_nn:
        out["nn"] = {"index": idx, "distance": dist}
        if method == "descent":
            out["nn"]["method"] = "descent"
    return out


def dpt(dm, root=None, roots=None, n_dcs=10, normalize=True):
    """Diffusion pseudotime from a diffmap*() result: dpt_r(i) = sqrt(sum_{l=1}^{n_dcs-1} (lambda_l / (1 - lambda_l))^2 (psi_l(r) -
    psi_l(i))^2).  root: one 0-based cell -> a vector of n values; roots: several -> n x len(roots), one call for all of them.  A
    root's own pseudotime is 0; cells outside the solved component get inf.  normalize: each root's values divided by their largest
    finite one.  2 <= n_dcs <= n_comps; a root must lie inside the solved component."""
    who = "dpt"
    if not isinstance(dm, dict) or "evals" not in dm or "evecs" not in dm:
        raise SharpError(f"{who}: dm must be what diffmap(), diffmap_neighbors() or diffmap_graph() returned")
    evals = np.ascontiguousarray(dm["evals"], np.float64)
    evecs = np.ascontiguousarray(dm["evecs"], np.float64)
    if evecs.ndim != 2 or evals.shape != (evecs.shape[1],) or not 2 <= evals.size <= MAX_COMPS:
        raise SharpError(f"{who}: evals (n_comps) and evecs (n x n_comps) do not fit, or n_comps is outside 2 .. {MAX_COMPS}")
    n, n_comps = evecs.shape
    if (root is None) == (roots is None):
        raise SharpError(f"{who}: give root or roots")
    if isinstance(n_dcs, bool) or int(n_dcs) != n_dcs or not 2 <= int(n_dcs) <= n_comps:
        raise SharpError(f"{who}: n_dcs must be an integer in 2 .. n_comps = {n_comps}")
    r = np.atleast_1d(np.asarray(root if roots is None else roots))
    if r.ndim != 1 or r.size < 1 or r.size > 4096 or not np.issubdtype(r.dtype, np.integer):
        raise SharpError(f"{who}: roots must be 1 .. 4096 integers")
    if r.min() < 0 or r.max() >= n:
        raise SharpError(f"{who}: a root out of range (the map has {n} rows, counted from 0)")
    if np.isnan(evecs[r, 0]).any():
        raise SharpError(f"{who}: root {int(r[np.isnan(evecs[r, 0])][0])} lies outside the component that was solved")
    if not (np.abs(evals[1:int(n_dcs)]) < 1.0).all():
        raise SharpError(f"{who}: an eigenvalue beyond the trivial one must lie inside (-1, 1)")
    r = np.ascontiguousarray(r, np.int32)
    _lib.ensure_init()
    out = np.zeros((n, r.size))
    check(lib().sharp_dpt(f64(evals), f64(evecs), n, n_comps, int(n_dcs), i32(r), int(r.size), int(bool(normalize)), f64(out)))
    return out[:, 0].copy() if roots is None else out


# ---- the stages one at a time (tests) -------------------------------------------------------------------------------------------------
def _csr(row_ptr, col, val):
    return np.ascontiguousarray(row_ptr, np.int64), np.ascontiguousarray(col, np.int32), np.ascontiguousarray(val, np.float64)


def _transitions(row_ptr, col, val, density_normalize=True):
    """(a, z) of a symmetric CSR (sharp_diffmap_transitions)"""
    rp, cc, vv = _csr(row_ptr, col, val)
    n = rp.size - 1
    _lib.ensure_init()
    a, z = np.zeros(n), np.zeros(n)
    check(lib().sharp_diffmap_transitions(i64(rp), i32(cc), f64(vv), n, int(bool(density_normalize)), f64(a), f64(z)))
    return a, z


def _component(row_ptr, col, val, n_comps=2, root=-1):
    """(label, components, (sub_row_ptr, sub_col, sub_val), new_id) (sharp_diffmap_component)"""
    rp, cc, vv = _csr(row_ptr, col, val)
    n = rp.size - 1
    _lib.ensure_init()
    srp, sc, sv, new_id = np.zeros(n + 1, np.int64), np.zeros(max(cc.size, 1), np.int32), np.zeros(max(cc.size, 1)), np.zeros(n, np.int32)
    label = C.c_int()
    comps, sn, snnz = C.c_longlong(), C.c_longlong(), C.c_longlong()
    check(lib().sharp_diffmap_component(i64(rp), i32(cc), f64(vv), n, int(n_comps), int(root), C.byref(label), C.byref(comps), C.byref(sn),
                                        C.byref(snnz), i64(srp), i32(sc), f64(sv), i32(new_id)))
    return label.value, comps.value, (srp[: sn.value + 1].copy(), sc[: snnz.value].copy(), sv[: snnz.value].copy()), new_id
