"""scrublet() and simulate_doublets(): doublet detection on raw counts, the step before everything else in
highly_variable_genes -> expression_pca -> knn -> louvain / umap.

A doublet is a droplet that caught two cells.  The method (Wolock, Lopez and Klein 2019) simulates doublets as the sum of two observed
cells, places them in the observed cells' PCA and scores every cell by the share of simulated doublets among its nearest neighbours.
The specification is the project's own: the preprocessing is this project's variable-gene selection and sparse PCA, the pairs come from
the library's 64-bit mix, and no parity with the scrublet or scanpy packages is claimed.  The simulated doublets are made on the GPU from
the resident copy of the observed cells, slab after slab; their matrix never exists as a whole.  A call is a pure function of its
arguments: two calls give the same bits, and so do one block and the same cells cut into several.  Computed by libsharp_hip.so
(csrc/doublets.hip); there is no CPU path.

The k-NN stages take at most 255 neighbours per row, and the method asks for k_adj = round(n_neighbors (1 + n_sim / n)) of them over the
observed and the simulated rows together.  The default n_neighbors is therefore min(round(0.5 sqrt(n)), the largest value whose k_adj
is <= 255): at the default ratio of 2 that cap is 85 and binds above 28900 cells.  An explicit n_neighbors beyond it is refused."""
import ctypes as C
import warnings

import numpy as np

from . import _lib
from ._lib import SharpError, check, f64, i32, i64, lib
from .expr_pca import _MAX_L, _blocks, _genes, _options, _pointers
from .tsne import _nn_method

__all__ = ["scrublet", "simulate_doublets"]

_WHO = "scrublet"
_NN_KEYS = ("n_projections", "max_candidates", "n_iters", "delta", "seed")
_NN_DEFAULTS = (8, 0, 12, 0.001, 10)


def _counts(scExp, who):
    """scExp as CSC blocks of raw counts: a negative or non-finite value is refused here, before the library sees anything"""
    blocks, m, n = _blocks(scExp, who, False)
    for q, b in enumerate(blocks):
        if b.nnz and b.data.min() < 0:
            c = int(np.searchsorted(b.indptr, np.flatnonzero(b.data < 0)[0], side="right")) - 1
            raise SharpError(f"{who}: a negative value where counts are expected (block {q + 1}, cell {c}, counted from 0)")
    return blocks, m, n


def _seed(seed, who):
    if isinstance(seed, (bool, np.bool_)) or int(seed) != seed or not 0 <= int(seed) < 2 ** 53:
        raise SharpError(f"{who}: seed must be a whole number in [0, 2^53)")
    return int(seed)


def _plan(n, sim_doublet_ratio=2.0, n_neighbors=None, who=_WHO):
    """(n_sim, n_neighbors, k_adj) of a call on n cells: sharp_doublet_plan.  n_sim = round(ratio n); n_neighbors None: the default
    min(round(0.5 sqrt(n)), the largest value whose k_adj <= 255 and <= n + n_sim - 1); k_adj = round(n_neighbors (1 + n_sim / n)).
    Needs no device."""
    ratio = float(sim_doublet_ratio)
    if not (np.isfinite(ratio) and ratio > 0):
        raise SharpError(f"{who}: sim_doublet_ratio must be finite and > 0")
    if n_neighbors is None:
        nn = 0
    else:
        if int(n_neighbors) != n_neighbors or int(n_neighbors) < 1:
            raise SharpError(f"{who}: n_neighbors must be >= 1 (None: the default)")
        nn = min(int(n_neighbors), 2 ** 31 - 1)
    n_sim, nn_out, k_adj = C.c_longlong(), C.c_int(), C.c_int()
    check(lib().sharp_doublet_plan(int(n), ratio, nn, C.byref(n_sim), C.byref(nn_out), C.byref(k_adj)))
    return n_sim.value, nn_out.value, k_adj.value


def _pairs(n, n_sim, seed=0):
    """the parents (n_sim, 2) int64 of the simulated doublets: sharp_doublet_pairs; a pure function of (n, n_sim, seed), no device"""
    parents = np.zeros((int(n_sim), 2), np.int64)
    check(lib().sharp_doublet_pairs(int(n), int(n_sim), _seed(seed, "doublet_pairs"), i64(parents)))
    return parents


def _parents(parents, n, who):
    p = np.ascontiguousarray(parents, np.int64)
    if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1:
        raise SharpError(f"{who}: parents must be an (n_sim, 2) array of cell indices, n_sim >= 1")
    if p.min() < 0 or p.max() >= n:
        raise SharpError(f"{who}: a parent outside [0, n) (doublet {int(np.flatnonzero(((p < 0) | (p >= n)).any(1))[0])}, counted from 0)")
    return p


def simulate_doublets(scExp, n_sim=None, seed=0, parents=None, max_doublets_per_slab=0, capacity=None):
    """The simulated doublets themselves, for inspection and tests (scrublet() never brings them to the host): {"parents" (n_sim, 2)
    int64, "counts" (scipy CSC, genes x n_sim: column s = column parents[s, 0] + column parents[s, 1] of scExp, genes ascending, a gene
    of both parents stored once), "cell_sum" (n_sim)}.  parents None: the pairs of (n, n_sim, seed) that scrublet() draws; n_sim None:
    2 n.  max_doublets_per_slab (0: the library's memory budget alone) only cuts the work into slabs; capacity (None: enough) is the
    room of the result's indices and values, and one that is too small is refused."""
    import scipy.sparse as sp

    who = "simulate_doublets"
    blocks, m, n = _counts(scExp, who)
    if n < 1:
        raise SharpError(f"{who}: need at least 1 cell in all")
    if parents is None:
        n_sim = 2 * n if n_sim is None else int(n_sim)
        if n_sim < 1:
            raise SharpError(f"{who}: need n_sim >= 1")
        parents = _pairs(n, n_sim, seed)
    p = _parents(parents, n, who)
    n_sim = p.shape[0]
    if int(max_doublets_per_slab) < 0:
        raise SharpError(f"{who}: max_doublets_per_slab must be >= 0")
    length = np.concatenate([np.diff(b.indptr) for b in blocks]).astype(np.int64)
    cap = int(length[p].sum()) if capacity is None else int(capacity)
    if cap < 0:
        raise SharpError(f"{who}: capacity must be >= 0")
    _lib.ensure_init()
    args, keep = _pointers(blocks)
    cp, ri, vx, cs = np.zeros(n_sim + 1, np.int64), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1)), np.zeros(n_sim)
    check(lib().sharp_doublet_synth_csc(*args, m, i64(p), n_sim, int(max_doublets_per_slab), cap, i64(cp), i32(ri), f64(vx), f64(cs)))
    del keep
    nnz = int(cp[-1])
    return {"parents": p, "counts": sp.csc_matrix((vx[:nnz], ri[:nnz], cp), shape=(m, n_sim)), "cell_sum": cs}


def _fit_parts(fit, m, who):
    """(loadings, center, scale, genes or None, n_genes, normalize_total, log1p) of a result of expression_pca() that fits blocks of m genes"""
    try:
        V, mu, sd = (np.ascontiguousarray(fit[key], np.float64) for key in ("loadings", "center", "scale"))
        total, log1p = _options(fit["normalize_total"], fit["log1p"], who)
        sub = fit.get("genes")
        m_fit = V.shape[0] if sub is None else int(fit["n_genes_in"])
    except (KeyError, TypeError, IndexError, AttributeError, ValueError):
        raise SharpError(f"{who}: pca must be what expression_pca() returned") from None
    if V.ndim != 2 or mu.shape != (V.shape[0],) or sd.shape != (V.shape[0],) or not 1 <= V.shape[1] <= _MAX_L:
        raise SharpError(f"{who}: the pca's loadings, center and scale do not belong together")
    if m_fit != m:
        raise SharpError(f"{who}: the pca was fitted on {m_fit} genes, the blocks have {m}")
    g, mk = _genes(sub, m, who)
    if g is not None and mk != V.shape[0]:
        raise SharpError(f"{who}: the pca's loadings, center and scale do not belong together")
    return V, mu, sd, g, mk, total, log1p


def _project(scExp, parents, fit, max_doublets_per_slab=0):
    """the simulated doublets' scores (n_sim, k) in a fit of expression_pca(): sharp_doublet_project_csc, the stage entry the tests use"""
    who = "doublet_project"
    blocks, m, n = _counts(scExp, who)
    p = _parents(parents, n, who)
    V, mu, sd, g, mk, total, log1p = _fit_parts(fit, m, who)
    _lib.ensure_init()
    args, keep = _pointers(blocks)
    out = np.zeros((p.shape[0], V.shape[1]))
    check(lib().sharp_doublet_project_csc(*args, m, i64(p), p.shape[0], total, int(log1p), f64(V), f64(mu), f64(sd), V.shape[1],
                                          None if g is None else i32(g), mk, int(max_doublets_per_slab), f64(out)))
    del keep
    return out


def _neighbor_counts(index, n_obs):
    """per row of index (rows, K) the entries >= n_obs, int32: sharp_doublet_neighbor_counts"""
    idx = np.ascontiguousarray(index, np.int32)
    if idx.ndim != 2:
        raise SharpError("doublet_neighbor_counts: index must be a (rows, K) array")
    _lib.ensure_init()
    out = np.zeros(idx.shape[0], np.int32)
    check(lib().sharp_doublet_neighbor_counts(i32(idx), idx.shape[0], idx.shape[1], int(n_obs), i32(out)))
    return out


def _score_table(k_adj, r, expected_doublet_rate):
    """the score of every neighbour count 0 .. k_adj: sharp_doublet_score_table; needs no device"""
    out = np.zeros(int(k_adj) + 1)
    check(lib().sharp_doublet_score_table(int(k_adj), float(r), float(expected_doublet_rate), f64(out)))
    return out


def _threshold(scores_obs, scores_sim, threshold=None):
    """sharp_doublet_threshold -> {"threshold" (None when none was found), "threshold_found", "predicted_doublets" (None then), the three
    rates, "passes"}; needs no device"""
    obs, sim = np.ascontiguousarray(scores_obs, np.float64), np.ascontiguousarray(scores_sim, np.float64)
    thr, found, passes = C.c_double(), C.c_int(), C.c_int()
    pred, rates = np.zeros(obs.size, np.int32), np.zeros(3)
    check(lib().sharp_doublet_threshold(f64(obs), obs.size, f64(sim), sim.size, float("nan") if threshold is None else float(threshold),
                                        C.byref(thr), C.byref(found), i32(pred), f64(rates), C.byref(passes)))
    have = not np.isnan(thr.value)
    return {"threshold": thr.value if have else None, "threshold_found": bool(found.value), "predicted_doublets": pred.astype(bool) if have else None,
            "detected_doublet_rate": float(rates[0]) if have else None, "detectable_doublet_fraction": float(rates[1]) if have else None,
            "overall_doublet_rate": float(rates[2]) if have else None, "passes": passes.value}


def scrublet(scExp, sim_doublet_ratio=2.0, expected_doublet_rate=0.1, n_neighbors=None, n_prin_comps=30, n_top_genes=2000, genes=None,
             pca=None, normalize_total=1e4, log1p=True, scale=True, threshold=None, nn_method="exact", nn_args=None, seed=0, ret_sim=False,
             max_doublets_per_slab=0):
    """Doublet scores of the cells of scExp (raw counts, genes x cells, as expression_pca takes them).
    n_sim = round(sim_doublet_ratio n) doublets are simulated, each the sum of two cells drawn independently (seed; a cell may meet
    itself).  Without pca, highly_variable_genes(n_top_genes) (or genes) and expression_pca(n_prin_comps, genes=..., normalize_total,
    log1p, scale) are fitted on the observed cells; with pca (a result of expression_pca) that fit is used as it is, with its own
    transform and gene subset.  The doublets go through the fit as any new cell would: on integer counts their scores are bit for bit
    expression_pca_transform of the summed columns.  Then the k_adj = round(n_neighbors (1 + n_sim / n)) nearest neighbours of every
    observed and simulated row (nn_method "exact" or "descent", the latter with nn_args = knn_descent's keywords), the count c of
    simulated ones among them, q = (c + 1) / (k_adj + 2) and the score q rho / r / (1 - rho - q (1 - rho - rho / r)) with r = n_sim / n
    and rho = expected_doublet_rate.
    k_adj must be <= 255 (the k-NN stages' limit) and <= n + n_sim - 1: the default n_neighbors is min(round(0.5 sqrt(n)), the largest
    value that fits), and an explicit n_neighbors beyond it is refused.
    threshold None: the minimum between the two modes of the simulated scores' smoothed 256-bin histogram; when the histogram never
    shows two modes a RuntimeWarning says so, and threshold, predicted_doublets and the rates are None.
    Returns {"doublet_scores" (n), "doublet_scores_sim" (n_sim), "predicted_doublets" (bool, n, or None), "threshold",
    "threshold_found", "detected_doublet_rate", "detectable_doublet_fraction", "overall_doublet_rate", "n_neighbors", "k_adj", "n_sim",
    "parents" (n_sim, 2), "genes" (the fit's gene subset, or None), "neighbor_counts" (n + n_sim, int: what the scores come from),
    "expected_doublet_rate", "sim_doublet_ratio"}; ret_sim adds "sim_pca" (n_sim, n_prin_comps), the doublets' PCA scores.
    max_doublets_per_slab (0: the library's memory budget alone) only cuts the doublets into slabs; no result depends on it."""
    who = _WHO
    rho = float(expected_doublet_rate)
    if not 0 < rho < 1:                                          # (false for NaN too)
        raise SharpError(f"{who}: expected_doublet_rate must lie in (0, 1)")
    seed = _seed(seed, who)
    thr = float("nan")
    if threshold is not None:
        thr = float(threshold)
        if not np.isfinite(thr):
            raise SharpError(f"{who}: threshold must be finite (None: find it)")
    method = 1 if _nn_method(nn_method, who) == "descent" else 0
    nn = None
    if nn_args:
        if method == 0:
            raise SharpError(f"{who}: nn_args belong to nn_method = \"descent\"")
        unknown = sorted(set(nn_args) - set(_NN_KEYS))
        if unknown:
            raise SharpError(f"{who}: nn_args holds {unknown}; knn_descent takes {list(_NN_KEYS)}")
        nn = np.array([0 if nn_args.get(key, dflt) is None else nn_args.get(key, dflt) for key, dflt in zip(_NN_KEYS, _NN_DEFAULTS)], np.float64)
    if int(max_doublets_per_slab) < 0:
        raise SharpError(f"{who}: max_doublets_per_slab must be >= 0")
    blocks, m, n = _counts(scExp, who)
    if n < 2:
        raise SharpError(f"{who}: need at least 2 cells in all")
    n_sim, _, _ = _plan(n, sim_doublet_ratio, n_neighbors, who)
    if pca is not None:
        if genes is not None:
            raise SharpError(f"{who}: genes belongs to the fit; with pca= the pca's own gene subset is used")
        V, mu, sd, g, mk, total, lg = _fit_parts(pca, m, who)
        try:
            S = np.ascontiguousarray(pca["scores"], np.float64)
        except (KeyError, TypeError, IndexError):
            raise SharpError(f"{who}: pca must be what expression_pca() returned") from None
        if S.shape != (n, V.shape[1]):
            raise SharpError(f"{who}: the pca's scores are {S.shape[0] if S.ndim == 2 else '?'} cells, the blocks have {n}")
        if not np.isfinite(S).all():
            raise SharpError(f"{who}: the pca's scores hold a value that is NaN or infinite")
        k, top = V.shape[1], 1
        fit = (f64(S), f64(V), f64(mu), f64(sd))
    else:
        total, lg = _options(normalize_total, log1p, who)
        k = int(n_prin_comps)
        if not 1 <= k <= _MAX_L:
            raise SharpError(f"{who}: need 1 <= n_prin_comps <= {_MAX_L}")
        g, mk = _genes(genes, m, who)
        if g is None and (int(n_top_genes) != n_top_genes or int(n_top_genes) < 1):
            raise SharpError(f"{who}: n_top_genes must be an integer >= 1")
        top = min(int(n_top_genes), 2 ** 31 - 1)
        fit = (None, None, None, None)
    _lib.ensure_init()
    args, keep = _pointers(blocks)
    N = n + n_sim
    sc, ss, pred, counts = np.zeros(n), np.zeros(n_sim), np.zeros(n, np.int32), np.zeros(N, np.int32)
    thr_out, found, rates, nn_out, k_adj = C.c_double(), C.c_int(), np.zeros(3), C.c_int(), C.c_int()
    parents = np.zeros((n_sim, 2), np.int64)
    genes_out, n_genes_out = np.zeros(max(mk if g is not None else min(top, m), 1), np.int32), C.c_int()
    sim_pca = np.zeros((n_sim, k)) if ret_sim else None
    check(lib().sharp_scrublet_csc(*args, m, float(sim_doublet_ratio), rho, 0 if n_neighbors is None else int(n_neighbors), k, top,
                                   None if g is None else i32(g), mk, *fit, total, int(lg), int(bool(scale)), thr, method,
                                   None if nn is None else f64(nn), seed, int(max_doublets_per_slab), f64(sc), f64(ss), i32(pred),
                                   C.byref(thr_out), C.byref(found), f64(rates), C.byref(nn_out), C.byref(k_adj), i64(parents),
                                   i32(genes_out), C.byref(n_genes_out), i32(counts), None if sim_pca is None else f64(sim_pca)))
    del keep
    have = not np.isnan(thr_out.value)
    if not have:
        warnings.warn(f"{who}: no threshold found: the histogram of the simulated doublets' scores never shows two modes; "
                      "predicted_doublets is None (pass threshold= after looking at doublet_scores_sim)", RuntimeWarning, stacklevel=2)
    out = {"doublet_scores": sc, "doublet_scores_sim": ss, "predicted_doublets": pred.astype(bool) if have else None,
           "threshold": thr_out.value if have else None, "threshold_found": bool(found.value),
           "detected_doublet_rate": float(rates[0]) if have else None, "detectable_doublet_fraction": float(rates[1]) if have else None,
           "overall_doublet_rate": float(rates[2]) if have else None, "n_neighbors": nn_out.value, "k_adj": k_adj.value, "n_sim": n_sim,
           "parents": parents, "genes": genes_out[:n_genes_out.value].astype(np.int64) if n_genes_out.value else None,
           "neighbor_counts": counts.astype(np.int64), "expected_doublet_rate": rho, "sim_doublet_ratio": float(sim_doublet_ratio)}
    if ret_sim:
        out["sim_pca"] = sim_pca
    return out
