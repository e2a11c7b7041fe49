"""highly_variable_genes(): variable-gene selection on raw counts, the step before expression_pca(genes=...).

A gene's variance is compared with the variance that genes of its mean usually have: log10(var) is fitted against log10(mean) by a local
quadratic (tricube weights, the nearest span * N genes), the counts are clipped at mean + sqrt(fitted variance * cells), and the
variance of the clipped, standardised counts ranks the genes.  This is the variance-stabilising selection that Seurat calls "vst" and
scanpy "seurat_v3", but the specification is the project's own: the local fit is evaluated directly at every gene, not through R's
interpolated loess surface, so no parity with either is claimed.  Every sum runs in an order that the input fixes: two calls give the
same bits, and so do one block and the same cells cut into several.  Computed by libsharp_hip.so (csrc/hvg.hip); there is no CPU
path."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SharpError, check, f64, i32, lib
from .expr_pca import _blocks, _pointers

__all__ = ["highly_variable_genes"]

_MAX_FIT = 2 ** 20


def _span(span, who):
    span = float(span)
    if not (np.isfinite(span) and 0 < span <= 1):
        raise SharpError(f"{who}: span must lie in (0, 1]")
    return span


def highly_variable_genes(scExp, n_top_genes=2000, span=0.3):
    """The n_top_genes most variable genes of raw counts (scExp as expression_pca takes it; no transform; a negative value is refused).
    Returns {"means", "variances" (gene_stats(scExp, None, False) bit for bit), "variances_expected" (the fitted variance at the gene's
    mean, 0 for a constant gene), "variances_norm" (the variance of the clipped, standardised counts), "rank" (0-based among the
    selected, -1 otherwise), "highly_variable" (bool per gene), "genes" (the selected indices, ascending, int64: what
    expression_pca(genes=...) takes), "n_selected" (min(n_top_genes, the genes that vary)), "span", "q" (the points of a local fit) and
    "degree_counts" (how many fits ended at degree 0, 1, 2)}.  Ties of variances_norm go to the lower gene; a constant gene is never
    selected."""
    who = "highly_variable_genes"
    span = _span(span, who)
    if int(n_top_genes) != n_top_genes or int(n_top_genes) < 1:
        raise SharpError(f"{who}: n_top_genes must be an integer >= 1")
    top = min(int(n_top_genes), 2 ** 31 - 1)
    blocks, m, n = _blocks(scExp, who, False)
    for q, b in enumerate(blocks):
        if b.nnz and b.data.min() < 0:
            c = int(np.searchsorted(b.indptr, np.flatnonzero(b.data < 0)[0], side="right")) - 1
            raise SharpError(f"{who}: a negative value where counts are expected (block {q + 1}, cell {c}, counted from 0)")
    if n < 2:
        raise SharpError(f"{who}: need at least 2 cells in all")
    _lib.ensure_init()
    args, keep = _pointers(blocks)
    mu, var, ve, vn = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros(m)
    rank, hv, genes = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(min(top, m), np.int32)
    ns, q, dc = C.c_int(), C.c_int(), np.zeros(3, np.int32)
    check(lib().sharp_expr_hvg_csc(*args, m, top, span, f64(mu), f64(var), f64(ve), f64(vn), i32(rank), i32(hv), i32(genes), C.byref(ns),
                                   C.byref(q), i32(dc)))
    del keep
    return {"means": mu, "variances": var, "variances_expected": ve, "variances_norm": vn, "rank": rank.astype(np.int64),
            "highly_variable": hv.astype(bool), "genes": genes[:ns.value].astype(np.int64), "n_selected": ns.value, "span": span,
            "q": q.value, "degree_counts": dc.astype(np.int64)}


def _loess(x, y, span=0.3):
    """sharp_hvg_loess on the caller's points -> (fit, bandwidth, degree): the stage entry the tests use"""
    who = "hvg_loess"
    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    if x.ndim != 1 or x.shape != y.shape or not 1 <= x.size <= _MAX_FIT:
        raise SharpError(f"{who}: need 1 <= npts <= {_MAX_FIT} points, x and y of one length")
    span = _span(span, who)
    _lib.ensure_init()
    fit, bw, deg = np.zeros(x.size), np.zeros(x.size), np.zeros(x.size, np.int32)
    check(lib().sharp_hvg_loess(f64(x), f64(y), x.size, span, f64(fit), f64(bw), i32(deg)))
    return fit, bw, deg
