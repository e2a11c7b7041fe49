"""rank_genes_groups(): which genes distinguish each group of cells from the rest, or from a reference group: the step
right after leiden() / louvain_snn().

Per (group, gene): a Wilcoxon rank-sum test (normal approximation, average ranks, the zeros one tie group) or Welch's t-test on the
values that expression_pca() sees (normalised, log-transformed), the Benjamini-Hochberg adjustment per group, the fold change, the
AUROC, the means and the shares of expressing cells, and each group's genes ordered by score.  The rank sums are exact integers and
every floating-point sum runs in an order that the input fixes: two calls give the same bits, and so do one block and the same cells
cut into several.  The specification is the project's own; no parity with scanpy's rank_genes_groups or Seurat's FindAllMarkers is
claimed.  Computed by libsharp_hip.so (csrc/rank_genes.hip); there is no CPU path."""
import numpy as np

from . import _lib
from ._lib import SharpError, check, f64, i32, i64, lib
from .expr_pca import _blocks, _genes, _options, _pointers

__all__ = ["rank_genes_groups"]

_MAX_GROUPS = 1024
_MAX_CELLS = 2097151
_METHODS = {"wilcoxon": 0, "t-test": 1}


def _group_codes(groups, n, reference, method, who):
    """(levels, int32 codes, sizes, the reference's code or -1): the refusals that need no device"""
    groups = np.asarray(groups)
    if groups.ndim != 1 or groups.shape[0] != n:
        raise SharpError(f"{who}: groups must hold one label per cell ({groups.size} labels, {n} cells)")
    levels, codes = np.unique(groups, return_inverse=True)
    G = int(levels.size)
    if G < 2:
        raise SharpError(f"{who}: need at least 2 groups")
    if G > _MAX_GROUPS:
        raise SharpError(f"{who}: at most {_MAX_GROUPS} groups are supported")
    if n > _MAX_CELLS:
        raise SharpError(f"{who}: need at most {_MAX_CELLS} cells in all")
    if isinstance(reference, str) and reference == "rest" and "rest" not in levels.tolist():
        ref = -1
    else:
        at = np.flatnonzero(levels == reference) if np.ndim(reference) == 0 else np.zeros(0, np.int64)
        if at.size != 1:
            raise SharpError(f"{who}: reference must be \"rest\" or one of the group labels (got {reference!r})")
        ref = int(at[0])
    sizes = np.bincount(codes, minlength=G).astype(np.int64)
    if method == "t-test":
        other = n - sizes if ref < 0 else np.full(G, sizes[ref])
        bad = np.flatnonzero((sizes < 2) | (other < 2))
        if bad.size:
            raise SharpError(f"{who}: t-test needs at least 2 cells in every tested group and in what it is tested against "
                             f"(group {levels[bad[0]]!r})")
    return levels, np.ascontiguousarray(codes, np.int32), sizes, ref


def rank_genes_groups(scExp, groups, method="wilcoxon", reference="rest", normalize_total=1e4, log1p=True, genes=None, tie_correct=True,
                      continuity=False, n_genes=None):
    """scExp: what expression_pca takes (a matrix or a list of blocks, genes x cells, scipy sparse or dense).  groups: one label of any
    kind per cell, in the blocks' order (np.unique orders them; 2 .. 1024 groups, at most 2 097 151 cells).  method: "wilcoxon" or
    "t-test" (Welch).  reference: "rest" (each group against all other cells) or one of the labels: every other group is then tested
    against that group alone, ranks are taken among the cells of the two groups, and the reference's own row is NaN.
    normalize_total, log1p, genes: exactly expression_pca's (a cell is normalised by its sum over all genes before the subset is
    applied; None / False: no transform, negative values are then allowed and rank below the zeros).  tie_correct, continuity: the
    Wilcoxon variance's tie term and the continuity correction of z.  n_genes: the length of the ordered lists (default: all).
    Returns {"groups" (the levels), "group_sizes", and G x m float64 arrays "scores" (z or t), "pvals" (two-sided), "pvals_adj"
    (Benjamini-Hochberg per group), "logfoldchanges" (log2 of the ratio of expm1(mean) + 1e-9 under log1p, of mean + 1e-9 otherwise),
    "auc" (U / (n_g n_ref)), "means", "means_ref", "pct", "pct_ref" (shares of cells with a non-zero value), "order" (G x n_genes int64:
    each group's genes by score descending, ties to the lower gene, NaN scores last; indices into the kept genes), "method",
    "reference", "genes" and the options}.  A block carries no gene names, so no "names" are returned."""
    who = "rank_genes_groups"
    if method not in _METHODS:
        raise SharpError(f"{who}: method must be \"wilcoxon\" or \"t-test\" (got {method!r})")
    total, log1p = _options(normalize_total, log1p, who)
    blocks, m, n = _blocks(scExp, who, total > 0 or log1p)
    levels, codes, sizes, ref = _group_codes(groups, n, reference, method, who)
    g, mk = _genes(genes, m, who)
    mk = mk if g is not None else m
    if n_genes is None:
        n_order = mk
    else:
        if int(n_genes) != n_genes or not 1 <= int(n_genes) <= mk:
            raise SharpError(f"{who}: n_genes must be an integer in 1 .. {mk} (the kept genes)")
        n_order = int(n_genes)
    G = int(levels.size)
    if G * mk >= 2 ** 32:
        raise SharpError(f"{who}: groups x genes must stay below 2^32")
    _lib.ensure_init()
    args, keep = _pointers(blocks)
    names = ("scores", "pvals", "pvals_adj", "logfoldchanges", "auc", "means", "means_ref", "pct", "pct_ref")
    out = {k: np.zeros((G, mk)) for k in names}
    gs, order = np.zeros(G, np.int64), np.zeros((G, n_order), np.int64)
    check(lib().sharp_rank_genes_csc(*args, m, i32(codes), G, _METHODS[method], ref, total, int(log1p), None if g is None else i32(g),
                                     0 if g is None else mk, int(bool(tie_correct)), int(bool(continuity)), n_order, i64(gs),
                                     *(f64(out[k]) for k in names), i64(order)))
    del keep
    res = {"groups": levels, "group_sizes": gs}
    res.update(out)
    res.update({"order": order, "method": method, "reference": "rest" if ref < 0 else levels[ref], "normalize_total": total if total > 0 else None,
                "log1p": log1p, "tie_correct": bool(tie_correct), "continuity": bool(continuity), "n_genes": n_order,
                "genes": None if g is None else g.astype(np.int64)})
    return res


def _rank_sums(scExp, codes, n_groups, reference=-1, normalize_total=1e4, log1p=True, genes=None, fill=-7):
    """sharp_rank_sums_csc on dense group codes -> (2R G x m, the tie terms (m for the rest, G x m for a reference), the non-zero counts
    G x m), int64, pre-filled with `fill`: the stage entry the tests use.  Nothing is refused here: the library's own checks answer."""
    who = "rank_sums"
    total, log1p = _options(normalize_total, log1p, who)
    blocks, m, n = _blocks(scExp, who, total > 0 or log1p)
    g, mk = _genes(genes, m, who)
    mk = mk if g is not None else m
    codes = np.ascontiguousarray(codes, np.int32)
    if codes.shape != (n,):
        raise SharpError(f"{who}: need one code per cell")
    G = max(int(n_groups), 1)
    _lib.ensure_init()
    args, keep = _pointers(blocks)
    r2 = np.full((G, mk), fill, np.int64)
    ties = np.full((G, mk) if reference >= 0 else (mk,), fill, np.int64)
    cnt = np.full((G, mk), fill, np.int64)
    check(lib().sharp_rank_sums_csc(*args, m, i32(codes), int(n_groups), int(reference), total, int(log1p), None if g is None else i32(g),
                                    0 if g is None else mk, i64(r2), i64(ties), i64(cnt)))
    del keep
    return r2, ties, cnt
