"""louvain(), louvain_neighbors(), louvain_snn(), louvain_graph(), their leiden*() counterparts and modularity(): a clustering read off
the neighbour graph.

The graph is the fuzzy union umap() builds from the k-NN lists -- scanpy's connectivities --, the shared-nearest-neighbour graph with
Jaccard weights that Seurat clusters (louvain_snn(), louvain(graph="snn"); snn_graph() returns it), or any symmetric CSR the caller
has.  The method is this project's own synchronous form of Louvain: weights are quantised to integers
once, so every sum of weights is exact whatever the order of the GPU's atomics; a round moves all vertices at once from the round's start
state, a hashed bit per community deciding whether it may lose or gain members in that round; a round is kept when the modularity rises.
A call is a pure function of its arguments: two calls give the same bits.  No parity with networkx, igraph or cuGraph is claimed.
leiden*() run the same levels with Leiden's refinement between a level's move phase and its aggregation: every community is
re-partitioned into well-connected sub-communities, those become the next level's vertices, and the next level starts from the
community partition, so parts of a community can still change sides; the returned communities are connected.  It is the project's own
deterministic form (no random choice among the candidates, one iteration); no parity with leidenalg, igraph or scanpy is claimed.
Computed by libsharp_hip.so (csrc/louvain.hip, csrc/leiden.hip); there is no CPU path."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SharpError, check, f64, i32, i64, lib
from .snn import PRUNE, _lists, _prune, _search
from .tsne import _neighbour_arrays

__all__ = ["louvain", "louvain_neighbors", "louvain_snn", "louvain_graph", "leiden", "leiden_neighbors", "leiden_snn", "leiden_graph",
           "modularity"]

_MAX_N = 16777216


def _limits(who, resolution, tol, max_levels, max_rounds, max_fails, seed):
    """the refusals of the arguments that need no device -> (resolution, tol, max_levels, max_rounds, max_fails, seed)"""
    resolution = float(resolution)
    if not (np.isfinite(resolution) and 0.0 < resolution <= 1e6):
        raise SharpError(f"{who}: resolution must be in (0, 1e6]")
    tol = float(tol)
    if not (np.isfinite(tol) and tol >= 0.0):
        raise SharpError(f"{who}: tol must be finite and >= 0")
    for name, v, hi in (("max_levels", max_levels, 64), ("max_rounds", max_rounds, 100000), ("max_fails", max_fails, 64)):
        if not 1 <= int(v) <= hi:
            raise SharpError(f"{who}: {name} must be in 1 .. {hi}")
    if not (np.isfinite(seed) and abs(seed) < 9.0e18 and float(seed) == int(seed)):
        raise SharpError(f"{who}: seed must be a finite integer")
    return resolution, tol, int(max_levels), int(max_rounds), int(max_fails), int(seed)


def _symmetric_csr(row_ptr, col, val, who):
    """(row_ptr int64, col int32, val float64) of a symmetric CSR without diagonal entries, refused by name otherwise"""
    rp = np.ascontiguousarray(row_ptr, np.int64)
    cc = np.asarray(col)
    vv = np.ascontiguousarray(val, np.float64)
    if rp.ndim != 1 or rp.size < 2 or cc.ndim != 1 or rp[0] != 0 or rp[-1] != cc.size:
        raise SharpError(f"{who}: row_ptr must hold n + 1 values from 0 to the number of entries of col")
    if vv.shape != cc.shape:
        raise SharpError(f"{who}: col and val must be vectors of one length")
    if not np.issubdtype(cc.dtype, np.integer):
        raise SharpError(f"{who}: col must hold integers, not {cc.dtype}")
    n = rp.size - 1
    if not 2 <= n <= _MAX_N:
        raise SharpError(f"{who}: need 2 <= n <= {_MAX_N} vertices")
    if cc.size == 0:
        raise SharpError(f"{who}: the graph holds no entry")
    if (np.diff(rp) < 0).any():
        raise SharpError(f"{who}: row_ptr is not monotone")
    if cc.min() < 0 or cc.max() >= n:
        raise SharpError(f"{who}: a column index out of range")
    cc = np.ascontiguousarray(cc, np.int32)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    if not (np.abs(vv) <= 1e100).all() or (vv < 0).any():                                 # (the first is false for NaN too)
        raise SharpError(f"{who}: a weight that is NA / NaN / Inf, negative or beyond 1e100")
    if (cc == row).any():
        raise SharpError(f"{who}: a diagonal entry (row {int(row[cc == row][0])}, counted from 0)")
    key = row * n + cc
    if (np.diff(key) <= 0).any():
        raise SharpError(f"{who}: the columns of a row must ascend strictly")
    tkey = cc.astype(np.int64) * n + row
    at = np.minimum(np.searchsorted(key, tkey), key.size - 1)
    if not (key[at] == tkey).all() or not (vv[at] == vv).all():
        raise SharpError(f"{who}: the graph is not symmetric")
    if not (vv > 0).any():
        raise SharpError(f"{who}: the graph holds no positive weight")
    return rp, cc, vv


class _Out:
    """the output buffers of a sharp_louvain_* or sharp_leiden_* call and the result dict made of them"""

    def __init__(self, n, max_levels, ret_levels, leiden):
        self.leiden = leiden
        self.mem = np.zeros(n, np.int32)
        self.ln, self.lc, self.ls = (np.zeros(max_levels, np.int64) for _ in range(3))
        self.lr, self.lf = np.zeros(max_levels, np.int32), np.zeros(max_levels, np.int32)
        self.lq = np.zeros(max_levels)
        self.lm = np.zeros((max_levels, n), np.int32) if ret_levels else None
        self.q, self.nl, self.cap = C.c_double(), C.c_int(), max_levels

    def args(self):
        if self.leiden:
            return (i32(self.mem), C.byref(self.q), self.cap, i64(self.ln), i64(self.lc), i64(self.ls), i32(self.lr), i32(self.lf),
                    f64(self.lq), C.byref(self.nl), i32(self.lm))
        return i32(self.mem), self.cap, i64(self.ln), i64(self.lc), i32(self.lr), f64(self.lq), C.byref(self.nl), i32(self.lm)

    def result(self, seed):
        levels = []
        for i in range(self.nl.value):
            lev = {"n": int(self.ln[i]), "communities": int(self.lc[i])}
            if self.leiden:
                lev["sub_communities"] = int(self.ls[i])
            lev["rounds"] = int(self.lr[i])
            if self.leiden:
                lev["refine_rounds"] = int(self.lf[i])
            lev["modularity"] = float(self.lq[i])
            if self.lm is not None:
                lev["membership"] = self.lm[i] + 1
            levels.append(lev)
        if self.leiden:                                       # of the returned membership, which the last level's P is split into
            communities, q = int(self.mem.max()), self.q.value
        else:
            communities, q = levels[-1]["communities"], levels[-1]["modularity"]
        return {"membership": self.mem, "n_communities": communities, "modularity": q, "levels": levels, "seed": seed}


def louvain_graph(row_ptr, col, val, resolution=1.0, seed=10, tol=1e-7, max_levels=20, max_rounds=200, max_fails=4, ret_levels=False):
    """Louvain on any symmetric weighted graph given as a CSR: row_ptr (n + 1), col (0-based, ascending within a row, no diagonal
    entry), val (finite, >= 0, <= 1e100, val[i, j] == val[j, i] bit for bit, at least one positive).  Returns {"membership" (int32,
    1 .. G by decreasing size, ties to the community with the smallest member), "n_communities", "modularity", "levels": [{"n",
    "communities", "rounds", "modularity"}, ...], "seed"}; with ret_levels each level also carries "membership" (1-based coarse
    vertices of the input's vertices, in ascending order of the communities' ids).  A level that merges nothing is recorded and ends
    the run.  resolution in (0, 1e6]; tol: the rise of the modularity a round must exceed to be kept; max_rounds rounds per level,
    max_fails discarded rounds in a row end a level."""
    who = "louvain_graph"
    a = _limits(who, resolution, tol, max_levels, max_rounds, max_fails, seed)
    rp, cc, vv = _symmetric_csr(row_ptr, col, val, who)
    n = rp.size - 1
    _lib.ensure_init()
    o = _Out(n, a[2], ret_levels, False)
    check(lib().sharp_louvain_graph(i64(rp), i32(cc), f64(vv), n, a[0], a[1], a[2], a[3], a[4], float(a[5]), *o.args()))
    return o.result(a[5])


def louvain_neighbors(index, distance, squared=False, resolution=1.0, seed=10, tol=1e-7, max_levels=20, max_rounds=200, max_fails=4,
                      ret_levels=False):
    """Louvain on the fuzzy graph of neighbour lists the caller already has -- what knn(X, K) returns: index (n x K, 0-based),
    distance (n x K) Euclidean, or their squares with squared=True.  The graph is umap_neighbors' (n_neighbors = K + 1), built on the
    device, and never leaves it.  The result is louvain_graph's."""
    who = "louvain_neighbors"
    a = _limits(who, resolution, tol, max_levels, max_rounds, max_fails, seed)
    index, distance = _neighbour_arrays(index, distance, who)
    n, K = index.shape
    if n > _MAX_N:
        raise SharpError(f"{who}: need 2 <= n <= {_MAX_N} rows")
    _lib.ensure_init()
    o = _Out(n, a[2], ret_levels, False)
    check(lib().sharp_louvain_neighbors(i32(index), f64(distance), n, int(K), int(bool(squared)), a[0], a[1], a[2], a[3], a[4], float(a[5]),
                                        *o.args()))
    return o.result(a[5])


def louvain_snn(index, prune=PRUNE, resolution=1.0, seed=10, tol=1e-7, max_levels=20, max_rounds=200, max_fails=4, ret_levels=False):
    """Louvain on the SNN graph of neighbour lists the caller already has (index: n x K, 0-based, what knn(X, K) returns; distances are
    not used): snn_graph(index, prune)'s graph with k = K + 1, built on the device, and never leaving it.  The result is
    louvain_graph's on that graph, bit for bit.  A prune that leaves no entry is refused."""
    who = "louvain_snn"
    a = _limits(who, resolution, tol, max_levels, max_rounds, max_fails, seed)
    prune = _prune(prune, who)
    index = _lists(index, who)
    n, K = index.shape
    _lib.ensure_init()
    o = _Out(n, a[2], ret_levels, False)
    check(lib().sharp_louvain_snn(i32(index), n, int(K), prune, a[0], a[1], a[2], a[3], a[4], float(a[5]), *o.args()))
    return o.result(a[5])


def _graph_choice(who, nn_method, nn_args, graph, prune):
    """the refusals of louvain()'s and leiden()'s search and graph arguments -> prune (graph = "snn": checked, None: 1/15)"""
    from .tsne import _nn_method

    method = _nn_method(nn_method, who)
    if nn_args and method != "descent":
        raise SharpError(f"{who}: nn_args belong to nn_method = \"descent\"")
    if graph not in ("fuzzy", "snn"):
        raise SharpError(f"{who}: graph must be \"fuzzy\" or \"snn\", not {graph!r}")
    if graph == "fuzzy" and prune is not None:
        raise SharpError(f"{who}: prune belongs to graph = \"snn\"")
    return _prune(PRUNE if prune is None else prune, who) if graph == "snn" else prune


def _on_rows(who, X, n_neighbors, nn_method, nn_args, pca, pca_center, graph, prune, ret_nn, ret_levels, limits, max_refine_rounds=None):
    """louvain()'s body, and with max_refine_rounds leiden()'s: the refusals, the search, the clustering of the lists' fuzzy or SNN graph"""
    prune = _graph_choice(who, nn_method, nn_args, graph, prune)
    a = _limits(who, *limits)
    kw = dict(resolution=a[0], seed=a[5], tol=a[1], max_levels=a[2], max_rounds=a[3], max_fails=a[4], ret_levels=ret_levels)
    on_snn, on_lists = louvain_snn, louvain_neighbors
    if max_refine_rounds is not None:
        kw["max_refine_rounds"] = _refine_limit(who, max_refine_rounds)
        on_snn, on_lists = leiden_snn, leiden_neighbors
    idx, dist, method = _search(X, n_neighbors, nn_method, nn_args, pca, pca_center, who)
    out = on_snn(idx, prune, **kw) if graph == "snn" else on_lists(idx, dist, **kw)
    if ret_nn:
        out["nn"] = {"index": idx, "distance": dist}
        if method == "descent":
            out["nn"]["method"] = "descent"
    return out


def louvain(X, n_neighbors=15, resolution=1.0, nn_method="exact", nn_args=None, pca=None, seed=10, tol=1e-7, max_levels=20,
            ret_levels=False, ret_nn=False, pca_center=True, max_rounds=200, max_fails=4, graph="fuzzy", prune=None):
    """Louvain on the neighbour graph of the rows of X, as sc.tl.louvain runs it on scanpy's connectivities.  The input is prepared and
    searched as umap() does it: pca None or a number of components (centred when pca_center), n_neighbors counts the row itself
    (2 .. 256, below n), nn_method "exact" or "descent" (knn_descent()'s approximate lists, nn_args its keywords).  The result is
    louvain_neighbors' on those lists; with ret_nn it also carries "nn": {"index", "distance"}.  graph="snn": the SNN / Jaccard graph
    of those lists instead (n_neighbors is Seurat's k.param; prune in [0, 1], None: 1/15) -- louvain_snn's result.  prune belongs to
    graph="snn"."""
    return _on_rows("louvain", X, n_neighbors, nn_method, nn_args, pca, pca_center, graph, prune, ret_nn, ret_levels,
                    (resolution, tol, max_levels, max_rounds, max_fails, seed))


# ---- Leiden ---------------------------------------------------------------------------------------------------------------------------
def _refine_limit(who, max_refine_rounds):
    if not 1 <= int(max_refine_rounds) <= 100000:
        raise SharpError(f"{who}: max_refine_rounds must be in 1 .. 100000")
    return int(max_refine_rounds)


def leiden_graph(row_ptr, col, val, resolution=1.0, seed=10, tol=1e-7, max_levels=20, max_rounds=200, max_fails=4, max_refine_rounds=200,
                 ret_levels=False):
    """Leiden on any symmetric weighted graph given as a CSR (louvain_graph's input and refusals).  Returns louvain_graph's dict:
    "membership" (int32, 1 .. G by decreasing size; every community is connected in the graph), "n_communities", "modularity" (of the
    membership: modularity() of it, bit for bit), "levels": [{"n", "communities" and "modularity" (of the level's partition P),
    "sub_communities" (what the refinement made of P: the next level's vertices), "rounds" (of the move phase), "refine_rounds"}, ...],
    "seed"; with ret_levels each level also carries "membership" (the 1-based rank of the community P of every input vertex).  The run
    ends at the first level whose refinement merges nothing, or at max_levels; the last level's P, split into its connected components,
    is returned.  max_refine_rounds (1 .. 100000): the cap on a level's refinement rounds."""
    who = "leiden_graph"
    a = _limits(who, resolution, tol, max_levels, max_rounds, max_fails, seed)
    mrr = _refine_limit(who, max_refine_rounds)
    rp, cc, vv = _symmetric_csr(row_ptr, col, val, who)
    n = rp.size - 1
    _lib.ensure_init()
    o = _Out(n, a[2], ret_levels, True)
    check(lib().sharp_leiden_graph(i64(rp), i32(cc), f64(vv), n, a[0], a[1], a[2], a[3], a[4], mrr, float(a[5]), *o.args()))
    return o.result(a[5])


def leiden_neighbors(index, distance, squared=False, resolution=1.0, seed=10, tol=1e-7, max_levels=20, max_rounds=200, max_fails=4,
                     max_refine_rounds=200, ret_levels=False):
    """Leiden on the fuzzy graph of neighbour lists the caller already has (louvain_neighbors' input): the graph is built on the device
    and never leaves it.  The result is leiden_graph's."""
    who = "leiden_neighbors"
    a = _limits(who, resolution, tol, max_levels, max_rounds, max_fails, seed)
    mrr = _refine_limit(who, max_refine_rounds)
    index, distance = _neighbour_arrays(index, distance, who)
    n, K = index.shape
    if n > _MAX_N:
        raise SharpError(f"{who}: need 2 <= n <= {_MAX_N} rows")
    _lib.ensure_init()
    o = _Out(n, a[2], ret_levels, True)
    check(lib().sharp_leiden_neighbors(i32(index), f64(distance), n, int(K), int(bool(squared)), a[0], a[1], a[2], a[3], a[4], mrr, float(a[5]),
                                       *o.args()))
    return o.result(a[5])


def leiden_snn(index, prune=PRUNE, resolution=1.0, seed=10, tol=1e-7, max_levels=20, max_rounds=200, max_fails=4, max_refine_rounds=200,
               ret_levels=False):
    """Leiden on the SNN graph of neighbour lists the caller already has (louvain_snn's input): snn_graph(index, prune)'s graph, built on
    the device.  The result is leiden_graph's on that graph, bit for bit."""
    who = "leiden_snn"
    a = _limits(who, resolution, tol, max_levels, max_rounds, max_fails, seed)
    mrr = _refine_limit(who, max_refine_rounds)
    prune = _prune(prune, who)
    index = _lists(index, who)
    n, K = index.shape
    _lib.ensure_init()
    o = _Out(n, a[2], ret_levels, True)
    check(lib().sharp_leiden_snn(i32(index), n, int(K), prune, a[0], a[1], a[2], a[3], a[4], mrr, float(a[5]), *o.args()))
    return o.result(a[5])


def leiden(X, n_neighbors=15, resolution=1.0, nn_method="exact", nn_args=None, pca=None, seed=10, tol=1e-7, max_levels=20,
           ret_levels=False, ret_nn=False, pca_center=True, max_rounds=200, max_fails=4, graph="fuzzy", prune=None, max_refine_rounds=200):
    """Leiden on the neighbour graph of the rows of X, as sc.tl.leiden runs it on scanpy's connectivities (graph="snn": as Seurat's
    FindClusters(algorithm = 4) on its SNN graph).  louvain()'s arguments, preparation and search; the result is leiden_neighbors' (or
    leiden_snn's) on those lists; with ret_nn it also carries "nn"."""
    return _on_rows("leiden", X, n_neighbors, nn_method, nn_args, pca, pca_center, graph, prune, ret_nn, ret_levels,
                    (resolution, tol, max_levels, max_rounds, max_fails, seed), max_refine_rounds)


def modularity(row_ptr, col, val, membership, resolution=1.0):
    """Q = sum_c [ in_c / 2m - resolution (tot_c / 2m)^2 ] of a labelling of a symmetric weighted CSR (louvain_graph's input), on the
    integer weights louvain uses and summed in its fixed order: modularity() of a louvain result's membership is the result's
    "modularity" bit for bit.  membership: n integer labels (any values)."""
    who = "modularity"
    resolution = _limits(who, resolution, 0.0, 1, 1, 1, 0)[0]
    rp, cc, vv = _symmetric_csr(row_ptr, col, val, who)
    n = rp.size - 1
    m = np.asarray(membership)
    if m.shape != (n,) or not np.issubdtype(m.dtype, np.integer):
        raise SharpError(f"{who}: membership must hold n integer labels")
    comm = np.ascontiguousarray(np.unique(m, return_inverse=True)[1].reshape(-1), np.int32)
    _lib.ensure_init()
    Q = C.c_double()
    check(lib().sharp_louvain_modularity(i64(rp), i32(cc), f64(vv), None, n, i32(comm), resolution, C.byref(Q)))
    return Q.value


# ---- the stages one at a time (tests) -------------------------------------------------------------------------------------------------
def _int_csr(row_ptr, col, q):
    return np.ascontiguousarray(row_ptr, np.int64), np.ascontiguousarray(col, np.int32), np.ascontiguousarray(q, np.int64)


def _row_caps():
    a, b = C.c_int(), C.c_int()
    check(lib().sharp_louvain_row_caps(C.byref(a), C.byref(b)))
    return a.value, b.value


def _quantise(row_ptr, col, val):
    """(q, k, 2m) of a float-weighted graph (sharp_louvain_quantise); q = 0 entries stay in place"""
    rp, cc = np.ascontiguousarray(row_ptr, np.int64), np.ascontiguousarray(col, np.int32)
    vv = np.ascontiguousarray(val, np.float64)
    n = rp.size - 1
    _lib.ensure_init()
    q, k, m2 = np.zeros(cc.size, np.int64), np.zeros(n, np.int64), C.c_longlong()
    check(lib().sharp_louvain_quantise(i64(rp), i32(cc), f64(vv), n, i64(q), i64(k), C.byref(m2)))
    return q, k, m2.value


def _move(row_ptr, col, q, comm, resolution=1.0, seed=10, level=0, rnd=0):
    """the proposals of one round on an integer-weighted CSR (sharp_louvain_move)"""
    rp, cc, qq = _int_csr(row_ptr, col, q)
    n = rp.size - 1
    comm = np.ascontiguousarray(comm, np.int32)
    _lib.ensure_init()
    prop = np.zeros(n, np.int32)
    check(lib().sharp_louvain_move(i64(rp), i32(cc) if cc.size else None, i64(qq) if qq.size else None, n, i32(comm), float(resolution),
                                   float(seed), int(level), int(rnd), i32(prop)))
    return prop


def _modularity_q(row_ptr, col, q, comm, resolution=1.0):
    """Q of a membership (ids in [0, n)) of an integer-weighted CSR (sharp_louvain_modularity)"""
    rp, cc, qq = _int_csr(row_ptr, col, q)
    n = rp.size - 1
    comm = np.ascontiguousarray(comm, np.int32)
    _lib.ensure_init()
    Q = C.c_double()
    check(lib().sharp_louvain_modularity(i64(rp), i32(cc), None, i64(qq), n, i32(comm), float(resolution), C.byref(Q)))
    return Q.value


def _aggregate(row_ptr, col, q, comm):
    """(row_ptr, col, q, new) of the coarse graph (sharp_louvain_aggregate)"""
    rp, cc, qq = _int_csr(row_ptr, col, q)
    n = rp.size - 1
    comm = np.ascontiguousarray(comm, np.int32)
    _lib.ensure_init()
    orp, oc, oq, new = np.zeros(n + 1, np.int64), np.zeros(cc.size, np.int32), np.zeros(cc.size, np.int64), np.zeros(n, np.int32)
    nnz, nc = C.c_longlong(), C.c_longlong()
    check(lib().sharp_louvain_aggregate(i64(rp), i32(cc), i64(qq), n, i32(comm), i64(orp), i32(oc), i64(oq), C.byref(nnz), C.byref(nc), i32(new)))
    return orp[: nc.value + 1].copy(), oc[: nnz.value].copy(), oq[: nnz.value].copy(), new


def _leiden_level(row_ptr, col, q, comm0, resolution=1.0, seed=10, level=0, tol=1e-7, max_rounds=200, max_fails=4):
    """(comm, rounds, Q): a level's move phase from comm0 (sharp_leiden_level)"""
    rp, cc, qq = _int_csr(row_ptr, col, q)
    n = rp.size - 1
    comm0 = np.ascontiguousarray(comm0, np.int32)
    _lib.ensure_init()
    comm, rounds, Q = np.zeros(n, np.int32), C.c_int(), C.c_double()
    check(lib().sharp_leiden_level(i64(rp), i32(cc) if cc.size else None, i64(qq) if qq.size else None, n, i32(comm0), float(resolution),
                                   float(tol), int(max_rounds), int(max_fails), float(seed), int(level), i32(comm), C.byref(rounds), C.byref(Q)))
    return comm, rounds.value, Q.value


def _leiden_refine(row_ptr, col, q, P, ref, resolution=1.0, seed=10, level=0, rnd=0):
    """(proposal, moved, wanting) of one refinement round from the state ref inside P (sharp_leiden_refine)"""
    rp, cc, qq = _int_csr(row_ptr, col, q)
    n = rp.size - 1
    P, ref = np.ascontiguousarray(P, np.int32), np.ascontiguousarray(ref, np.int32)
    _lib.ensure_init()
    prop, moved, wanting = np.zeros(n, np.int32), C.c_longlong(), C.c_longlong()
    check(lib().sharp_leiden_refine(i64(rp), i32(cc) if cc.size else None, i64(qq) if qq.size else None, n, i32(P), i32(ref), float(resolution),
                                    float(seed), int(level), int(rnd), i32(prop), C.byref(moved), C.byref(wanting)))
    return prop, moved.value, wanting.value


def _leiden_split(row_ptr, col, q, label):
    """(out, count): the components inside a labelling, named by their smallest vertex (sharp_leiden_split)"""
    rp, cc, qq = _int_csr(row_ptr, col, q)
    n = rp.size - 1
    label = np.ascontiguousarray(label, np.int32)
    _lib.ensure_init()
    out, count = np.zeros(n, np.int32), C.c_longlong()
    check(lib().sharp_leiden_split(i64(rp), i32(cc) if cc.size else None, i64(qq) if qq.size else None, n, i32(label), i32(out), C.byref(count)))
    return out, count.value
