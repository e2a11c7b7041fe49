"""Literal numpy restatements used by the tree / plot_markers tests: hclust.f's HCASS2 (R's merge matrix and leaf order from the
(ia, ib) list), the selection part of R/plot_markers.R:46-151 and R/get_percluster_exp.R:24-78.  Test infrastructure."""
import math

import numpy as np


def hcass2(ia, ib):
    """hclust.f, SUBROUTINE HCASS2: returns merge ((n - 1, 2)) and order (n), as R's hclust object holds them"""
    ia, ib = np.asarray(ia, np.int64), np.asarray(ib, np.int64)
    n = ia.size + 1
    iia, iib = ia.copy(), ib.copy()
    for i in range(n - 2):                                   # DO I = 1, N-2: later uses of the cluster formed at step I point to -I
        k = min(ia[i], ib[i])
        t = np.arange(i + 1, n - 1)
        iia[t[ia[t] == k]] = -(i + 1)
        iib[t[ib[t] == k]] = -(i + 1)
    iia, iib = -iia, -iib                                    # singletons negative, clusters positive
    for i in range(n - 1):
        if iia[i] > 0 and iib[i] < 0:
            iia[i], iib[i] = iib[i], iia[i]
        if iia[i] > 0 and iib[i] > 0:
            iia[i], iib[i] = min(iia[i], iib[i]), max(iia[i], iib[i])
    iorder = [int(iia[n - 2]), int(iib[n - 2])]
    for i in range(n - 3, -1, -1):                           # DO I = N-2, 1, -1: replace step I + 1 by its two members
        j = iorder.index(i + 1)
        iorder[j] = int(iia[i])
        iorder.insert(j + 1, int(iib[i]))
    return np.stack([iia, iib], 1).astype(np.int32), (-np.asarray(iorder)).astype(np.int32)


def leaves(merge):
    """list of leaf arrays (1-based observations) per merge row"""
    out = []
    for a, b in merge:
        la = np.array([-a]) if a < 0 else out[a - 1]
        lb = np.array([-b]) if b < 0 else out[b - 1]
        out.append(np.concatenate([la, lb]))
    return out


def cut(merge, k):
    """labels of the partition into k clusters after the first n - k merges (ids arbitrary)"""
    n = merge.shape[0] + 1
    lab = np.zeros(n, np.int64)
    lv = leaves(merge[: n - k])
    done = np.zeros(n, bool)
    cid = 0
    for i in range(n - k - 1, -1, -1):
        m = lv[i] - 1
        if not done[m[0]]:
            cid += 1
            lab[m] = cid
            done[m] = True
    for i in np.flatnonzero(~done):
        cid += 1
        lab[i] = cid
    return lab


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return len(set(zip(a.tolist(), b.tolist()))) == len(set(a.tolist())) == len(set(b.tolist()))


def r_rank(v):
    v = np.asarray(v, np.float64)
    return np.array([np.sum(v < x) + (np.sum(v == x) + 1) / 2.0 for x in v])


def plot_markers_select(sginfo, label=None, N_marker=10, sN_cluster=None, nratio=None, logmark=None):
    """R/plot_markers.R:46-151 line by line (tables as dicts of columns)"""
    if label is None:
        label = sginfo["label"]
    label = np.asarray(label)
    if nratio is None:
        nratio = 1e4 / len(label)
    mg = sginfo["mginfo"]
    nrow = len(mg["icluster"])
    d = sorted(range(nrow), key=lambda i: (mg["icluster"][i], mg["pvalue"][i]))                       # :57
    rk = r_rank([mg["auc"][i] for i in d])
    o = sorted(range(nrow), key=lambda j: (mg["icluster"][d[j]], -rk[j], mg["pvalue"][d[j]]))          # :61
    srows = [d[j] for j in o]
    kk = sorted(set(int(c) for c in mg["icluster"]))
    if sN_cluster is None:
        sN_cluster = len(kk)
    kk = kk[:sN_cluster]                                                                              # :75
    ss = []
    for c in kk:                                                                                       # :91-95
        x = [r for r in srows if mg["icluster"][r] == c]
        ss += x[: min(len(x), N_marker)]
    cellind = sorted(range(len(label)), key=lambda i: label[i])                                        # order(): stable
    newc = label[cellind]
    sm = np.asarray(sginfo["mat"], np.float64)[ss][:, cellind]
    scind = [i for i in range(len(newc)) if newc[i] in kk]
    cells = [cellind[i] for i in scind]
    newc, sm = newc[scind], sm[:, scind]
    if len(cellind) > 1e4:                                                                             # :136-143
        ki = []
        for u in list(dict.fromkeys(newc.tolist())):
            w = [i for i in range(len(newc)) if newc[i] == u]
            ki += w[: int(math.ceil(len(w) * nratio))]
        cells, newc, sm = [cells[i] for i in ki], newc[ki], sm[:, ki]
    if logmark is None:
        logmark = sginfo["logmark"]
    my = np.log2(sm + 1) if logmark else sm
    keep = [i for i in range(my.shape[0]) if np.std(my[i], ddof=1) != 0]
    my = my[keep]
    my = np.array([(r - r.mean()) / np.std(r, ddof=1) for r in my]).reshape(len(keep), my.shape[1])
    return {"sortmarker_rows": srows, "sm": my, "genes": [mg["gene"][ss[i]] for i in keep], "cells": cells}


def percluster(blocks, labels):
    """R/get_percluster_exp.R:39-66 on dense blocks: per cluster (sorted unique labels) the columns in block order, then cell order"""
    labels = np.asarray(labels)
    out, off = {int(u): [] for u in sorted(set(labels.tolist()))}, 0
    for b in blocks:
        for j in range(b.shape[1]):
            out[int(labels[off + j])].append(b[:, j])
        off += b.shape[1]
    return [np.stack(v, 1) if v else None for v in out.values()]
