"""harmony_integrate(): a Harmony-style batch integration of PCA scores, the step between expression_pca() and the
neighbour search.

A soft k-means on the unit rows of the scores whose assignment penalises clusters that one batch fills, followed by a ridge correction
per cluster that takes each batch's offset out of the original scores; the two alternate until the clustering objective settles.  It
is modelled on Harmony (Korsunsky et al. 2019) for one categorical covariate, but the specification is the project's own: the cells are
dealt to blocks and the start cells are picked by a hash of the seed, and every sum runs in an order that the input's shape fixes, so
two calls give the same bits.  No parity with the Harmony packages is claimed.  Computed by libsharp_hip.so (csrc/harmony.hip); there
is no CPU path."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SharpError, check, f64, i32, lib

__all__ = ["harmony_integrate", "batch_of_blocks"]

_MAX_D, _MAX_K, _MAX_B, _MAX_BLOCKS, _MAX_N = 128, 256, 4096, 1024, 2 ** 31 - 2


def batch_of_blocks(blocks):
    """The block number (0-based, int64) of every cell of a list of genes x cells blocks, in the order in which expression_pca() stacks
    their cells: the batch labels of harmony_integrate() when every block is a sample, donor or run."""
    if hasattr(blocks, "shape"):
        blocks = [blocks]
    return np.repeat(np.arange(len(blocks), dtype=np.int64), [int(b.shape[1]) for b in blocks])


def _matrix(Z, who, name="Z"):
    Z = np.ascontiguousarray(Z, np.float64)
    if Z.ndim != 2 or not 1 <= Z.shape[0] <= _MAX_N:
        raise SharpError(f"{who}: {name} must be a matrix of 1 <= n <= 2^31 - 2 rows")
    if not np.isfinite(Z).all():
        raise SharpError(f"{who}: a non-finite value in {name} (row {int(np.flatnonzero(~np.isfinite(Z).all(axis=1))[0])}, counted from 0)")
    return Z


def _shape(who, n, d, K, B):
    if not 2 <= d <= _MAX_D:
        raise SharpError(f"{who}: need 2 <= d <= {_MAX_D} columns")
    if B == 1:
        raise SharpError(f"{who}: one batch: nothing to integrate")
    if not 2 <= B <= _MAX_B:
        raise SharpError(f"{who}: need 2 <= batches <= {_MAX_B}")
    if K > n:
        raise SharpError(f"{who}: n_clusters exceeds the number of cells")
    if not 2 <= K <= _MAX_K:
        raise SharpError(f"{who}: need 2 <= n_clusters <= min(n, {_MAX_K})")


def _codes(batch, n, B, who):
    """dense codes as the library takes them: within [0, B), every code present"""
    batch = np.ascontiguousarray(batch)
    if batch.shape != (n,) or batch.dtype.kind not in "iu":
        raise SharpError(f"{who}: batch must hold one integer code per cell")
    if batch.min() < 0 or batch.max() >= B:
        raise SharpError(f"{who}: a batch code outside [0, batches) (cell {int(np.flatnonzero((batch < 0) | (batch >= B))[0])}, counted from 0)")
    cnt = np.bincount(batch, minlength=B)
    if (cnt == 0).any():
        raise SharpError(f"{who}: an empty batch code ({int(np.flatnonzero(cnt == 0)[0])})")
    return batch.astype(np.int32)


def harmony_integrate(Z, batch, n_clusters=None, sigma=0.1, theta=2.0, lam=1.0, max_iter=10, max_iter_cluster=20, n_blocks=20,
                      epsilon_cluster=1e-5, epsilon_harmony=1e-4, init_iter=10, seed=1, ret_R=False):
    """Z (n x d scores, 2 <= d <= 128, finite, no zero row) with the batches' offsets taken out.  batch: one label per cell, of any kind
    (np.unique orders them; at least two, at most 4096).  n_clusters: default min(round(n / 30), 100), within 2 .. min(n, 256).
    sigma > 0: the softness of the assignment; theta >= 0: the weight of the batch-diversity penalty (0: plain soft k-means); lam > 0: the
    ridge penalty of the correction.  Up to max_iter corrections, each after up to max_iter_cluster clustering rounds over n_blocks
    hashed blocks of cells; a clustering stops when a round lowers the objective by less than epsilon_cluster of it, the whole when an
    iteration does by less than epsilon_harmony (0: every round runs).  init_iter Lloyd rounds on the cosine start the centroids.
    Returns {"Z_corr" (n x d, the rows in Z's order), "Y" (the centroids, unit rows), "objective" (one per iteration), "rounds" (the
    clustering rounds of each), "n_iter", "converged", "n_clusters", "n_batches", "batch_levels", and "R" (n x n_clusters, the soft
    assignment) with ret_R}."""
    who = "harmony_integrate"
    Z = _matrix(Z, who)
    n, d = Z.shape
    batch = np.asarray(batch)
    if batch.shape != (n,):
        raise SharpError(f"{who}: batch must hold one label per cell")
    levels, codes = np.unique(batch, return_inverse=True)
    B = int(levels.size)
    K = min(int(round(n / 30)), 100) if n_clusters is None else n_clusters
    if int(K) != K:
        raise SharpError(f"{who}: n_clusters must be an integer")
    K = int(K)
    _shape(who, n, d, K, B)
    for name, v, ok in (("sigma", sigma, lambda x: x > 0), ("theta", theta, lambda x: x >= 0), ("lam", lam, lambda x: x > 0),
                        ("epsilon_cluster", epsilon_cluster, lambda x: x >= 0), ("epsilon_harmony", epsilon_harmony, lambda x: x >= 0)):
        if not (np.isfinite(float(v)) and ok(float(v))):
            raise SharpError(f"{who}: {name} must be " + ("> 0" if name in ("sigma", "lam") else ">= 0"))
    if not 1 <= int(n_blocks) <= _MAX_BLOCKS:
        raise SharpError(f"{who}: need 1 <= n_blocks <= {_MAX_BLOCKS}")
    if int(max_iter) < 1 or int(max_iter_cluster) < 1 or int(init_iter) < 0:
        raise SharpError(f"{who}: need max_iter >= 1, max_iter_cluster >= 1, init_iter >= 0")
    zero = np.flatnonzero(~Z.any(axis=1))
    if zero.size:
        raise SharpError(f"{who}: a zero row in Z (cell {int(zero[0])}, counted from 0)")
    codes = _codes(codes.reshape(-1), n, B, who)
    _lib.ensure_init()
    max_iter = int(max_iter)
    Zc, Y = np.zeros((n, d)), np.zeros((K, d))
    obj, rounds = np.zeros(max_iter), np.zeros(max_iter, np.int32)
    n_iter, conv = C.c_int(), C.c_int()
    R = np.zeros((n, K)) if ret_R else None
    check(lib().sharp_harmony(f64(Z), n, d, i32(codes), B, K, float(sigma), float(theta), float(lam), max_iter, int(max_iter_cluster),
                              int(n_blocks), float(epsilon_cluster), float(epsilon_harmony), int(init_iter), int(seed), f64(Zc), f64(Y),
                              f64(obj), i32(rounds), C.byref(n_iter), C.byref(conv), f64(R)))
    out = {"Z_corr": Zc, "Y": Y, "objective": obj[:n_iter.value].copy(), "rounds": rounds[:n_iter.value].astype(np.int64),
           "n_iter": n_iter.value, "converged": bool(conv.value), "n_clusters": K, "n_batches": B, "batch_levels": levels}
    if ret_R:
        out["R"] = R
    return out


def _caps():
    """(the cells of a slab of the sums, the doubles of Y that the assign kernel stages at a time); needs no device"""
    slab, tile = C.c_int(), C.c_int()
    check(lib().sharp_harmony_caps(C.byref(slab), C.byref(tile)))
    return slab.value, tile.value


def _assign(Zhat, Y, batch, P=None, sigma=0.1, i0=0, i1=None, argmax=False, out=None):
    """sharp_harmony_assign on the caller's arrays -> R (n x K; the rows outside [i0, i1) as `out` holds them, zero without it), or
    a (int32) in argmax mode: the stage entry the tests use"""
    who = "harmony_assign"
    Zhat, Y = _matrix(Zhat, who, "Zhat"), _matrix(Y, who, "Y")
    n, d = Zhat.shape
    K = Y.shape[0]
    B = int(np.max(batch)) + 1 if P is None else np.asarray(P).shape[0]
    if Y.shape[1] != d:
        raise SharpError(f"{who}: Zhat and Y must have the same columns")
    _shape(who, n, d, K, B)
    codes = _codes(batch, n, B, who)
    if P is not None:
        P = _matrix(P, who, "P")
        if P.shape != (B, K):
            raise SharpError(f"{who}: P must be batches x n_clusters")
    i1 = n if i1 is None else i1
    _lib.ensure_init()
    if argmax:
        a = np.full(n, -1, np.int32) if out is None else np.ascontiguousarray(out, np.int32).copy()
        check(lib().sharp_harmony_assign(f64(Zhat), f64(Y), i32(codes), f64(P), n, d, K, B, int(i0), int(i1), float(sigma), 1, None, i32(a)))
        return a
    R = np.zeros((n, K)) if out is None else np.ascontiguousarray(out, np.float64).copy()
    check(lib().sharp_harmony_assign(f64(Zhat), f64(Y), i32(codes), f64(P), n, d, K, B, int(i0), int(i1), float(sigma), 0, f64(R), None))
    return R


def _sums(R, X, batch, B, seed=1, n_blocks=20):
    """sharp_harmony_sums -> (O (n_blocks x B x K), S (B x K x d))"""
    who = "harmony_sums"
    R, X = _matrix(R, who, "R"), _matrix(X, who, "X")
    n, K = R.shape
    d = X.shape[1]
    if X.shape[0] != n:
        raise SharpError(f"{who}: R and X must have the same rows")
    _shape(who, n, d, K, B)
    if not 1 <= int(n_blocks) <= _MAX_BLOCKS:
        raise SharpError(f"{who}: need 1 <= n_blocks <= {_MAX_BLOCKS}")
    codes = _codes(batch, n, B, who)
    _lib.ensure_init()
    O, S = np.zeros((int(n_blocks), B, K)), np.zeros((B, K, d))
    check(lib().sharp_harmony_sums(f64(R), f64(X), i32(codes), n, d, K, B, int(seed), int(n_blocks), f64(O), f64(S)))
    return O, S


def _correct(Z, R, batch, W):
    """sharp_harmony_correct -> Z_corr (n x d); W: B x K x d"""
    who = "harmony_correct"
    Z, R = _matrix(Z, who), _matrix(R, who, "R")
    W = np.ascontiguousarray(W, np.float64)
    n, d = Z.shape
    K = R.shape[1]
    if R.shape[0] != n or W.ndim != 3 or W.shape[1:] != (K, d) or not np.isfinite(W).all():
        raise SharpError(f"{who}: need R n x K and a finite W batches x K x d")
    B = W.shape[0]
    _shape(who, n, d, K, B)
    codes = _codes(batch, n, B, who)
    _lib.ensure_init()
    out = np.zeros((n, d))
    check(lib().sharp_harmony_correct(f64(Z), f64(R), i32(codes), f64(W), n, d, K, B, f64(out)))
    return out


def _ridge(N, S, lam=1.0):
    """sharp_harmony_ridge -> W (B x K x d) from N (B x K) and S (B x K x d): the library's own host function; needs no device"""
    who = "harmony_ridge"
    N, S = np.ascontiguousarray(N, np.float64), np.ascontiguousarray(S, np.float64)
    if N.ndim != 2 or S.ndim != 3 or S.shape[:2] != N.shape:
        raise SharpError(f"{who}: need N batches x n_clusters and S batches x n_clusters x d")
    B, K, d = S.shape
    W = np.zeros((B, K, d))
    check(lib().sharp_harmony_ridge(f64(N), f64(S), B, K, d, float(lam), f64(W)))
    return W
