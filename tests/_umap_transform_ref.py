"""The umap_transform specification of DESIGN.md §14 in numpy fp64: the lists of a query against a reference, sigma / weights / start,
one epoch and a full transform, plus the inputs and quality measures the tests share.  This is the project's own specification (modelled
on umap-learn's transform and uwot's umap_transform); it claims no bit parity with either.  The GPU tests compare every stage of
libsharp_hip.so with these functions on the stage's own input."""
import numpy as np

import _umap_ref as ref

KS = (15, 64, 65, 255)
DS = (3, 10, 50, 70)
# (share, ratio) of quality() for the reference fit (ref.run on blobs(), seed 10) and the reference transform of full_run_queries() with
# the seeds 10, 1, 2, 3, 4 (tests/test_umap_transform_cpu.py runs them): recorded in DESIGN.md §14, the yardstick of the GPU's full run
REF_QUALITY = {10: (1.0, 1.5537972027811222), 1: (1.0, 1.343675122592587), 2: (1.0, 1.302487230370182),
               3: (0.9983333333333333, 7.817616714273606), 4: (1.0, 1.603084132263201)}
_SH, _RA = [v[0] for v in REF_QUALITY.values()], [v[1] for v in REF_QUALITY.values()]
# §13's margin rule: the minimum less three spreads (2 / 600 where the spread is 0), the maximum plus three spreads
SHARE_FLOOR = min(_SH) - (3 * (max(_SH) - min(_SH)) if max(_SH) > min(_SH) else 2 / 600)
RATIO_CEILING = max(_RA) + 3 * (max(_RA) - min(_RA))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def reference_rows(d, n=1025):
    """the tests' reference: (X_ref, labels)"""
    return ref.blobs(n, d, 6, 0)


def queries(X_ref, lab, nq=333, seed=7):
    """nq rows drawn as N(0, 1) around the per-label means of the reference: (Xq, labels)"""
    rng = np.random.default_rng(seed)
    k = int(lab.max()) + 1
    means = np.stack([X_ref[lab == c].mean(0) for c in range(k)])
    ql = np.arange(nq) % k
    return means[ql] + rng.normal(size=(nq, X_ref.shape[1])), ql


# ---- lists ----------------------------------------------------------------------------------------------------------------------------
def direct_d2(X_ref, q):
    """sum_c (q_c - x_jc)^2 for every reference row j"""
    t = np.asarray(X_ref, np.float64) - np.asarray(q, np.float64)
    return (t * t).sum(1)


def cross_knn(X_ref, Xq, K):
    """the K nearest reference rows of every query row, nothing excluded, sorted by (distance, index): (idx, Euclidean distances)"""
    X_ref = np.asarray(X_ref, np.float64)
    Xq = np.asarray(Xq, np.float64)
    n = X_ref.shape[0]
    idx = np.zeros((Xq.shape[0], K), np.int64)
    d = np.zeros((Xq.shape[0], K))
    for q in range(Xq.shape[0]):
        d2 = direct_d2(X_ref, Xq[q])
        o = np.lexsort((np.arange(n), d2))[:K]
        idx[q], d[q] = o, np.sqrt(d2[o])
    return idx, d


def gap_ratio(X_ref, Xq, K):
    """per query row: (the (K + 1)-th smallest squared distance - the K-th) / (||q - mu||^2 + max_j ||x_j - mu||^2): the selection on
    the GEMM form ||q - mu||^2 + ||w_j||^2 - 2 (q - mu).w_j errs by a few eps times that scale, so a gap well above it means the GEMM
    form and the direct sum select the same K rows"""
    X_ref = np.asarray(X_ref, np.float64)
    mu = X_ref.mean(0)
    wmax = ((X_ref - mu) ** 2).sum(1).max()
    out = np.zeros(Xq.shape[0])
    for q in range(Xq.shape[0]):
        d2 = np.sort(direct_d2(X_ref, Xq[q]))
        out[q] = (d2[K] - d2[K - 1]) / (((Xq[q] - mu) ** 2).sum() + wmax)
    return out


# ---- weights and start ----------------------------------------------------------------------------------------------------------------
def row_sum_at(d_row, sigma):
    with np.errstate(under="ignore", over="ignore", divide="ignore", invalid="ignore"):
        return np.exp(-np.asarray(d_row, np.float64) / sigma).sum()


def smooth(d):
    """sigma, the weights w (nq x K), the bisection's iterate mid and its step counts from the lists' Euclidean distances: rho = 0,
    target log2 K, the floor 1e-3 * the row's own mean distance"""
    d = np.asarray(d, np.float64)
    nq, K = d.shape
    target = np.log2(K)
    sigma, mids, steps = np.zeros(nq), np.zeros(nq), np.zeros(nq, np.int64)
    for q in range(nq):
        lo, hi, mid = 0.0, np.inf, 1.0
        it = 0
        while it < 64:
            s = row_sum_at(d[q], mid)
            if abs(s - target) < 1e-5:
                break
            if s > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if hi == np.inf else (lo + hi) / 2.0
            it += 1
        steps[q], mids[q] = it, mid
        sigma[q] = max(mid, 1e-3 * (d[q].sum() / K))
    return sigma, weights(d, sigma), mids, steps


def weights(d, sigma):
    with np.errstate(under="ignore", over="ignore"):
        return np.exp(-np.asarray(d, np.float64) / np.asarray(sigma)[:, None])


def start(idx, w, Y_ref):
    """y_q = sum_j w_qj Y_ref[idx_qj] / sum_j w_qj; a row whose weights all underflow starts at its nearest reference row"""
    Y_ref = np.asarray(Y_ref, np.float64)
    sw = w.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = (w[:, :, None] * Y_ref[idx]).sum(1) / sw[:, None]
    return np.where((sw > 0)[:, None], y, Y_ref[idx[:, 0]])


# ---- epochs ---------------------------------------------------------------------------------------------------------------------------
def epoch(idx, w, Y, Y_ref, ep, E, a, b, learning_rate=1.0, negative_sample_rate=5, repulsion_strength=1.0, seed=10, row_offset=0,
          return_terms=False):
    """Y (nq x dims) after epoch ep of E; return_terms: also the number of terms every row received and the number of coordinates the
    clip acted on.  Slot p of row q is edge (row_offset + q) K + p with rate w_qp; no factor 2, no self test; Y_ref is fixed."""
    Y = np.asarray(Y, np.float64)
    Y_ref = np.asarray(Y_ref, np.float64)
    idx = np.asarray(idx, np.int64)
    nq, K = idx.shape
    alpha = learning_rate * (1.0 - ep / E)
    rows = np.repeat(np.arange(nq, dtype=np.int64), K)
    f = np.nonzero(ref.fires(ep, np.asarray(w, np.float64).reshape(-1)))[0]
    delta = np.zeros_like(Y)
    terms = np.zeros(nq, np.int64)
    clipped = 0
    if f.size:
        i, j = rows[f], idx.reshape(-1)[f]
        edge = ((int(row_offset) + i) * K + (f % K)).astype(np.uint64)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
            diff = Y[i] - Y_ref[j]
            D = (diff * diff).sum(1)
            c = np.where(D > 0, (-2.0 * a * b * D ** (b - 1.0)) / (a * D ** b + 1.0), 0.0)
            g = np.where((D > 0)[:, None], np.clip(c[:, None] * diff, -4.0, 4.0), 0.0)
            clipped += int((np.abs(c[:, None] * diff)[D > 0] > 4.0).sum())
            np.add.at(delta, i, g)
            np.add.at(terms, i, 1)
            for s in range(negative_sample_rate):
                k = ref.draw(seed, ep, edge, s, Y_ref.shape[0])
                diff = Y[i] - Y_ref[k]
                D = (diff * diff).sum(1)
                ok = D > 0
                c = (2.0 * repulsion_strength * b) / ((0.001 + D) * (a * D ** b + 1.0))
                g = np.where(ok[:, None], np.clip(c[:, None] * diff, -4.0, 4.0), 0.0)
                clipped += int((np.abs(c[:, None] * diff)[ok] > 4.0).sum())
                np.add.at(delta, i, g)
                np.add.at(terms, i, 1)
    out = Y + alpha * delta
    return (out, terms, clipped) if return_terms else out


def transform(X_ref, Y_ref, Xq, n_neighbors, a, b, fit_epochs, n_epochs=None, learning_rate=1.0, negative_sample_rate=5,
              repulsion_strength=1.0, seed=10, row_offset=0):
    """the full reference transform"""
    E = fit_epochs // 3 if n_epochs is None else n_epochs
    idx, d = cross_knn(X_ref, Xq, n_neighbors)
    _, w, _, _ = smooth(d)
    Y = start(idx, w, Y_ref)
    for ep in range(E):
        Y = epoch(idx, w, Y, Y_ref, ep, E, a, b, learning_rate, negative_sample_rate, repulsion_strength, seed, row_offset)
    return Y


# ---- the full run's input and quality ---------------------------------------------------------------------------------------------------
def full_run_queries(nq=600, seed=11):
    """600 new rows of the six blobs of ref.blobs(1500, 10, 6, 0) (the same centres, fresh noise): (Xq, labels)"""
    centres = np.random.default_rng(0).normal(0.0, 6.0, size=(6, 10))       # blobs()'s first draw
    lab = np.arange(nq) % 6
    return centres[lab] + np.random.default_rng(seed).normal(size=(nq, 10)), lab


def quality(Y_ref, lab_ref, Yq, lab_q):
    """(the share of queries whose nearest reference point in the map carries their label; the largest ratio, over the blobs, of the
    farthest query from the blob's map centroid to the farthest reference point from it)"""
    Y_ref = np.asarray(Y_ref, np.float64)
    Yq = np.asarray(Yq, np.float64)
    near = np.array([np.argmin(((Y_ref - y) ** 2).sum(1)) for y in Yq])
    share = float((lab_ref[near] == lab_q).mean())
    ratios = []
    for c in range(int(lab_ref.max()) + 1):
        cen = Y_ref[lab_ref == c].mean(0)
        ratios.append(np.sqrt(((Yq[lab_q == c] - cen) ** 2).sum(1).max()) / np.sqrt(((Y_ref[lab_ref == c] - cen) ** 2).sum(1).max()))
    return share, float(max(ratios))
