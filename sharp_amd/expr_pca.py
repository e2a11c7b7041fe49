"""expression_pca(), expression_pca_transform() and gene_stats(): a truncated PCA of sparse expression blocks, the first
step of normalise -> log1p -> centre and scale -> PCA -> neighbours -> graph clustering or map.

scExp is what SHARP_unlimited takes: one matrix or a list of blocks, genes x cells, scipy sparse (CSC as it stands, anything else
converted) or dense (converted to CSC on the host), all with the same genes.  Centring and scaling are implicit: nothing dense of the
size cells x genes exists anywhere.  The fit is a randomised subspace iteration; its leading components converge, the components in
the noise do not, as for any randomised PCA.  Every sum runs in an order that the input's shape fixes: two calls give the same bits,
and so do one block and the same cells cut into several.  The specification is the project's own; no parity with sklearn, scanpy,
Seurat or irlba is claimed.  Computed by libsharp_hip.so (csrc/expr_pca.hip); there is no CPU path."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SharpError, check, f64, i32, i64, lib
from .api import _csc_int_slots, _csc_pointer_lists, _is_sparse

__all__ = ["expression_pca", "expression_pca_transform", "gene_stats"]

_MAX_L = 128
_MAX_M = 16777216
_MAX_N = 2 ** 31 - 2


def _blocks(scExp, who, check_neg):
    """scExp as a list of CSC blocks with float64 values and sorted indices; the refusals that need no device"""
    import scipy.sparse as sp

    if _is_sparse(scExp) or isinstance(scExp, np.ndarray):
        scExp = [scExp]
    try:
        blocks = list(scExp)
    except TypeError:
        raise SharpError(f"{who}: scExp must be a matrix or a list of matrices, genes x cells") from None
    if not blocks:
        raise SharpError(f"{who}: No expression data is provided!")
    out = []
    for q, b in enumerate(blocks):
        if _is_sparse(b):
            b = b.tocsc()
            if b.dtype != np.float64:
                b = b.astype(np.float64)
            if not b.has_sorted_indices:
                b = b.sorted_indices()
        else:
            b = np.asarray(b)
            if b.ndim != 2:
                raise SharpError(f"{who}: block {q + 1} must be a matrix, genes x cells")
            b = sp.csc_matrix(np.asarray(b, np.float64))
        if out and b.shape[0] != out[0].shape[0]:
            raise SharpError(f"{who}: every block must have the same genes (block {q + 1} has {b.shape[0]}, block 1 has {out[0].shape[0]})")
        if b.nnz and not np.isfinite(b.data).all():
            c = int(np.searchsorted(b.indptr, np.flatnonzero(~np.isfinite(b.data))[0], side="right")) - 1
            raise SharpError(f"{who}: a value that is NaN or infinite (block {q + 1}, cell {c}, counted from 0)")
        if check_neg and b.nnz and b.data.min() < 0:
            c = int(np.searchsorted(b.indptr, np.flatnonzero(b.data < 0)[0], side="right")) - 1
            raise SharpError(f"{who}: a negative value under normalize_total / log1p (block {q + 1}, cell {c}, counted from 0)")
        out.append(b)
    m = out[0].shape[0]
    n = sum(b.shape[1] for b in out)
    if not 1 <= m <= _MAX_M:
        raise SharpError(f"{who}: need 1 <= m <= {_MAX_M} genes")
    if n > _MAX_N:
        raise SharpError(f"{who}: need at most 2^31 - 2 cells in all")
    return out, m, n


def _options(normalize_total, log1p, who):
    total = 0.0 if normalize_total is None or normalize_total is False else float(normalize_total)
    if not (np.isfinite(total) and total >= 0):
        raise SharpError(f"{who}: normalize_total must be None or a positive number")
    return total, bool(log1p)


def _pointers(blocks):
    """the block-list arguments of the *_csc entries; the arrays are returned too, so that they live as long as the call"""
    cps, ris = _csc_int_slots(blocks)
    vxs = [np.ascontiguousarray(b.data, np.float64) for b in blocks]
    ncb = np.array([b.shape[1] for b in blocks], np.int64)
    return _csc_pointer_lists(cps, ris, vxs) + (i64(ncb), len(blocks)), (cps, ris, vxs, ncb)


def _genes(genes, m, who):
    """genes= as the library takes it: (None, 0) for all genes, else (a strictly ascending int32 array within [0, m), its length); a bool
    mask of length m stands for the indices it marks.  Unsorted, repeated, out-of-range and empty genes are refused by name."""
    if genes is None:
        return None, 0
    g = np.asarray(genes)
    if g.ndim != 1:
        raise SharpError(f"{who}: genes must be a one-dimensional array of gene indices or a bool mask of length m")
    if g.dtype == np.bool_:
        if g.size != m:
            raise SharpError(f"{who}: the genes mask has {g.size} entries, the blocks have {m} genes")
        g = np.flatnonzero(g)
    elif g.size and not np.issubdtype(g.dtype, np.integer):
        raise SharpError(f"{who}: genes must hold integers or be a bool mask")
    if g.size == 0:
        raise SharpError(f"{who}: genes is empty (it must keep at least one gene)")
    g = g.astype(np.int64)
    if g.min() < 0 or g.max() >= m:
        raise SharpError(f"{who}: genes holds an index outside [0, m) (position {int(np.flatnonzero((g < 0) | (g >= m))[0])}, counted from 0)")
    d = np.diff(g)
    if (d <= 0).any():                                          # (the first offending position decides the name, as in the library)
        at = int(np.flatnonzero(d <= 0)[0])
        what = "holds a gene twice" if d[at] == 0 else "must be ascending"
        raise SharpError(f"{who}: genes {what} (position {at + 1}, counted from 0)")
    return np.ascontiguousarray(g, np.int32), int(g.size)


def _row_caps():
    """(the entries of a gene that one wave sums, the rows of a slab of the Gram): sharp_expr_row_caps; needs no device"""
    a, b = C.c_int(), C.c_int()
    check(lib().sharp_expr_row_caps(C.byref(a), C.byref(b)))
    return a.value, b.value


def expression_pca(scExp, n_components=50, oversample=10, n_iter=4, normalize_total=1e4, log1p=True, center=True, scale=False, seed=0,
                   genes=None):
    """The n_components leading principal components of the cells.  Each cell is scaled to normalize_total counts (None: not), log1p is
    taken (log1p=False: not), every gene is centred and, with scale, divided by its standard deviation (a constant gene gets weight 0).
    l = n_components + oversample columns (at most 128, at most min(cells, genes)) are iterated n_iter times; seed picks the start.
    Returns {"scores" (cells x n_components, float64: the cells projected on the components, what knn, umap(pca=None), louvain and snn
    take, and what expression_pca_transform gives for the same cells), "loadings" (genes x n_components, orthonormal columns, each
    one's largest entry positive), "singular_values", "sdev" (singular values / sqrt(cells -
    1)), "center", "scale" (1 without scale), "gene_var", "total_var", and the options}.  Input of rank below l is refused:
    "numerical rank below n_components + oversample".
    genes (strictly ascending indices, or a bool mask of length m; e.g. highly_variable_genes()["genes"]) fits the PCA on those genes
    alone: the cells are normalised by their sums over ALL genes, then the other genes are dropped on the device.  loadings, center,
    scale and gene_var then have one row per kept gene, and the fit carries "genes", "n_genes_in" (m) and "n_genes" (the kept)."""
    who = "expression_pca"
    if not center:
        raise SharpError(f"{who}: center = False is not supported (an uncentred variant is out of scope)")
    total, log1p = _options(normalize_total, log1p, who)
    k, oversample, n_iter, seed = int(n_components), int(oversample), int(n_iter), int(seed)
    if k < 1:
        raise SharpError(f"{who}: n_components must be >= 1")
    if oversample < 0:
        raise SharpError(f"{who}: oversample must be >= 0")
    if k + oversample > _MAX_L:
        raise SharpError(f"{who}: n_components + oversample must be <= {_MAX_L}")
    if not 0 <= n_iter <= 1000:
        raise SharpError(f"{who}: n_iter must be in 0 .. 1000")
    if not 0 <= seed < 2 ** 63:
        raise SharpError(f"{who}: seed must be in 0 .. 2^63 - 1")
    blocks, m, n = _blocks(scExp, who, total > 0 or log1p)
    if n < 2:
        raise SharpError(f"{who}: need at least 2 cells in all")
    g, mk = _genes(genes, m, who)
    mk = mk if g is not None else m
    if k + oversample > min(n, mk):
        raise SharpError(f"{who}: n_components + oversample must be <= min(cells, genes)")
    _lib.ensure_init()
    args, keep = _pointers(blocks)
    scores, loadings = np.zeros((n, k)), np.zeros((mk, k))
    sv, sdev, mu, sd, var, tv = np.zeros(k), np.zeros(k), np.zeros(mk), np.zeros(mk), np.zeros(mk), C.c_double()
    out = (f64(scores), f64(loadings), f64(sv), f64(sdev), f64(mu), f64(sd), f64(var), C.byref(tv))
    if g is None:
        check(lib().sharp_expr_pca_csc(*args, m, k, oversample, n_iter, total, int(log1p), int(bool(scale)), seed, *out))
    else:
        check(lib().sharp_expr_pca_sub_csc(*args, m, k, oversample, n_iter, total, int(log1p), int(bool(scale)), seed, *out, i32(g), mk))
    del keep
    return {"scores": scores, "loadings": loadings, "singular_values": sv, "sdev": sdev, "center": mu, "scale": sd, "gene_var": var,
            "total_var": tv.value, "n_components": k, "oversample": oversample, "n_iter": n_iter,
            "normalize_total": total if total > 0 else None, "log1p": log1p, "centered": True, "scaled": bool(scale), "seed": seed,
            "n_cells": n, "n_genes": mk, "n_genes_in": m, "genes": None if g is None else g.astype(np.int64)}


def expression_pca_transform(scExp_new, fit):
    """The scores of new cells in a fit of expression_pca(): the cells go through the fit's transform, centre, scale and loadings.  A
    cell's row depends on that cell and the fit alone, so block-wise calls give the bits of one call.  A fit on a gene subset
    (fit["genes"]) takes new cells with all fit["n_genes_in"] genes and drops the others as the fit did."""
    who = "expression_pca_transform"
    try:
        V, mu, sd = (np.ascontiguousarray(fit[key], np.float64) for key in ("loadings", "center", "scale"))
        total, log1p = _options(fit["normalize_total"], fit["log1p"], who)
    except (KeyError, TypeError, IndexError):
        raise SharpError(f"{who}: fit must be what expression_pca() returned") from None
    if V.ndim != 2 or mu.shape != (V.shape[0],) or sd.shape != (V.shape[0],) or not 1 <= V.shape[1] <= _MAX_L:
        raise SharpError(f"{who}: the fit's loadings, center and scale do not belong together")
    blocks, m, n = _blocks(scExp_new, who, total > 0 or log1p)
    sub = fit.get("genes") if hasattr(fit, "get") else None
    m_fit = V.shape[0] if sub is None else fit.get("n_genes_in")
    if sub is not None and (not isinstance(m_fit, (int, np.integer)) or m_fit < 1):
        raise SharpError(f"{who}: fit must be what expression_pca() returned")
    if m != m_fit:
        raise SharpError(f"{who}: the new cells have {m} genes, the fit has {m_fit}")
    g, mk = _genes(sub, m, who)
    if g is not None and mk != V.shape[0]:
        raise SharpError(f"{who}: the fit's loadings, center and scale do not belong together")
    k = V.shape[1]
    scores = np.zeros((n, k))
    if n == 0:
        return scores
    _lib.ensure_init()
    args, keep = _pointers(blocks)
    if g is None:
        check(lib().sharp_expr_pca_transform_csc(*args, m, total, int(log1p), f64(V), f64(mu), f64(sd), k, f64(scores)))
    else:
        check(lib().sharp_expr_pca_transform_sub_csc(*args, m, total, int(log1p), f64(V), f64(mu), f64(sd), k, f64(scores), i32(g), mk))
    del keep
    return scores


def gene_stats(scExp, normalize_total=1e4, log1p=True, genes=None):
    """Per gene, after the transform of expression_pca(): {"mean", "var" (n - 1 in the denominator), "nnz" (cells with a non-zero
    value)}, and per cell "cell_sum".  mean and var are the fit's center and gene_var bit for bit.  genes (as in expression_pca):
    the statistics of those genes alone, the bits of the full call's rows; cell_sum stays the sum over all genes."""
    who = "gene_stats"
    total, log1p = _options(normalize_total, log1p, who)
    blocks, m, n = _blocks(scExp, who, total > 0 or log1p)
    if n < 2:
        raise SharpError(f"{who}: need at least 2 cells in all")
    g, mk = _genes(genes, m, who)
    mk = mk if g is not None else m
    _lib.ensure_init()
    args, keep = _pointers(blocks)
    mu, var, nnz, cs = np.zeros(mk), np.zeros(mk), np.zeros(mk, np.int64), np.zeros(n)
    if g is None:
        check(lib().sharp_expr_stats_csc(*args, m, total, int(log1p), f64(mu), f64(var), i64(nnz), f64(cs)))
    else:
        check(lib().sharp_expr_stats_sub_csc(*args, m, total, int(log1p), f64(mu), f64(var), i64(nnz), f64(cs), i32(g), mk))
    del keep
    return {"mean": mu, "var": var, "nnz": nnz, "cell_sum": cs, "normalize_total": total if total > 0 else None, "log1p": log1p}
