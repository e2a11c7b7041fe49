"""The approximate k-NN of DESIGN.md §16 in numpy fp64: the start from sorted random projections, the sampled reverse lists, one join and
a full run, with the brute-force lists to measure recall against.  This is the project's own specification; it claims no parity with
pynndescent or uwot.  Every distance is the direct sum s = 0; s += (x_ic - x_jc)^2 for c = 0 .. d-1 (a column loop here), and a list is
the K best distinct rows of everything it was offered, ordered by (distance, index): the GPU tests compare libsharp_hip.so with these
functions bit for bit, each stage on its own input."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
NONE = np.int64(2 ** 31 - 1)        # "no candidate" inside offer(): sorts behind every row index


def mix64(z):
    """the splitmix64 finaliser on uint64 arrays (arithmetic mod 2^64)"""
    z = np.asarray(z, np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def _u64(v):
    return np.asarray(v, np.uint64)


def default_candidates(K):
    return min(int(K), 30)


# ---- inputs the tests share -----------------------------------------------------------------------------------------------------------
def blobs(n, d, seed, centres=6):
    rng = np.random.default_rng(seed)
    mu = rng.normal(size=(centres, d)) * 6.0
    return np.ascontiguousarray(mu[rng.integers(0, centres, size=n)] + rng.normal(size=(n, d)))


def gaussian(n, d, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).normal(size=(n, d)))


def random_lists(n, K, seed):
    """well-formed lists that know nothing of X: K distinct rows other than the row itself"""
    rng = np.random.default_rng(seed)
    out = np.empty((n, K), np.int32)
    for i in range(n):
        c = rng.choice(n - 1, size=K, replace=False)
        out[i] = c + (c >= i)
    return out


DS = (3, 10, 50, 70)                                              # below, at and above a panel of 16 columns, and no multiple of it
KS = (15, 90, 255)
STAGE_CASES = [(d, K) for d in DS for K in KS]
FULL_INPUTS = ("blobs", "gaussian")


def stage_input(d):
    """1 025 rows (no multiple of 64, 16 or 4) for the stage tests"""
    return blobs(1025, d, 100 + d)


def full_input(name):
    return {"blobs": lambda: blobs(1025, 10, 1), "gaussian": lambda: gaussian(1025, 50, 2), "blobs20011": lambda: blobs(20011, 10, 3)}[name]()


def planted_duplicates(d, K=15):
    """the stage input with rows 700 and 701 made copies of row 3, and random lists in which row 3 names 701 before 700: after a join
    both sit at distance 0 in row 3's list (and each other's), the lower index first"""
    X = stage_input(d).copy()
    X[700] = X[3]
    X[701] = X[3]
    lists = random_lists(X.shape[0], K, 31)
    row = [v for v in lists[3] if v not in (700, 701)][: K - 2]
    lists[3] = np.array([701, 700] + row, np.int32)
    return X, lists


# ---- distances and lists --------------------------------------------------------------------------------------------------------------
def pair_dist2(X, I, J):
    """sum_c (X[I, c] - X[J, c])^2, column after column"""
    s = np.zeros(np.broadcast(I, J).shape)
    for c in range(X.shape[1]):
        col = X[:, c]
        t = col[I] - col[J]
        s += t * t
    return s


def offer(X, K, cand, row0=0):
    """Rows row0 .. row0 + len(cand) - 1: the K best distinct rows of cand (r x m, -1: none; the row itself is dropped) by
    (distance, index) -> (idx (r, K) int32, dist2 (r, K))."""
    C = np.asarray(cand, np.int64)
    rows = np.arange(row0, row0 + C.shape[0], dtype=np.int64)[:, None]
    C = np.where((C < 0) | (C == rows), NONE, C)
    C = np.sort(C, axis=1)
    valid = C != NONE
    valid[:, 1:] &= C[:, 1:] != C[:, :-1]
    D = np.where(valid, pair_dist2(X, np.broadcast_to(rows, C.shape), np.where(valid, C, 0)), np.inf)
    o = np.argsort(D, axis=1, kind="stable")[:, :K]               # (C ascends along a row: equal distances stay by the lower index)
    idx, dist = np.take_along_axis(C, o, 1), np.take_along_axis(D, o, 1)
    assert np.isfinite(dist).all(), "a row was offered fewer than K distinct rows"
    return idx.astype(np.int32), dist


def brute(X, K, chunk=512):
    """the exact lists: every other row offered"""
    n = X.shape[0]
    idx, dist = np.empty((n, K), np.int32), np.empty((n, K))
    allrows = np.arange(n, dtype=np.int64)[None, :]
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        idx[r0:r1], dist[r0:r1] = offer(X, K, np.broadcast_to(allrows, (r1 - r0, n)), r0)
    return idx, dist


def lists_of(X, index, chunk=4096):
    """given indices (any order) measured and sorted"""
    index = np.asarray(index)
    n, K = index.shape
    idx, dist = np.empty((n, K), np.int32), np.empty((n, K))
    for r0 in range(0, n, chunk):
        idx[r0:r0 + chunk], dist[r0:r0 + chunk] = offer(X, K, index[r0:r0 + chunk], r0)
    return idx, dist


def recall(idx, exact_idx):
    n, K = idx.shape
    hit = sum(np.intersect1d(idx[i], exact_idx[i], assume_unique=True).size for i in range(n))
    return hit / float(n * K)


# ---- start ----------------------------------------------------------------------------------------------------------------------------
def directions(seed, T, d):
    """r_t[c] in (-1, 1): ((mix(mix(seed GOLDEN + t) + c) >> 12) + 0.5) 2^-51 - 1"""
    with np.errstate(over="ignore"):
        bt = mix64(_u64(seed) * GOLDEN + np.arange(T, dtype=np.uint64))
        h = mix64(bt[:, None] + np.arange(d, dtype=np.uint64)[None, :])
    return ((h >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -51 - 1.0


def orders(X, T, seed):
    """(order, pos), each T x n: rows sorted by (p_t, index), and every row's position in that order"""
    n, d = X.shape
    R = directions(seed, T, d)
    order = np.empty((T, n), np.int64)
    pos = np.empty((T, n), np.int64)
    for t in range(T):
        p = np.zeros(n)
        for c in range(d):
            p += X[:, c] * R[t, c]
        order[t] = np.lexsort((np.arange(n), p))
        pos[t, order[t]] = np.arange(n)
    return order, pos


def start(X, K, T=8, seed=10, chunk=4096):
    n = X.shape[0]
    W = K
    order, pos = orders(X, T, seed)
    off = np.concatenate([np.arange(-W, 0), np.arange(1, W + 1)])
    idx, dist = np.empty((n, K), np.int32), np.empty((n, K))
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        cand = []
        for t in range(T):
            q = pos[t, r0:r1, None] + off[None, :]
            ok = (q >= 0) & (q < n)
            cand.append(np.where(ok, order[t][np.clip(q, 0, n - 1)], -1))
        idx[r0:r1], dist[r0:r1] = offer(X, K, np.concatenate(cand, 1), r0)
    return idx, dist


# ---- join -----------------------------------------------------------------------------------------------------------------------------
def candidates(idx, S, iteration, seed):
    """A (n x (min(K, S) + S), -1 padded): each row's first min(K, S) forward neighbours, then its at most S reverse neighbours of
    lowest hashed priority (ties to the lower source); and every row's full reverse degree."""
    idx = np.asarray(idx, np.int64)
    n, K = idx.shape
    Sf = min(K, S)
    v = np.repeat(np.arange(n, dtype=np.int64), K)
    u = idx.ravel()
    with np.errstate(over="ignore"):
        base = mix64(_u64(seed) * GOLDEN + _u64(iteration))
        pr = mix64(mix64(base + u.astype(np.uint64)) + v.astype(np.uint64)) >> np.uint64(32)
    o = np.lexsort((v, pr, u))
    us, vs = u[o], v[o]
    first = np.searchsorted(us, np.arange(n))
    rank = np.arange(us.size) - first[us]
    keep = rank < S
    A = np.full((n, Sf + S), -1, np.int64)
    A[:, :Sf] = idx[:, :Sf]
    A[us[keep], Sf + rank[keep]] = vs[keep]
    return A, np.bincount(u, minlength=n)


def join(X, idx, S=None, iteration=1, seed=10, chunk=1024):
    """one join from sorted lists -> (idx, dist2, entries that changed)"""
    idx = np.asarray(idx)
    n, K = idx.shape
    S = default_candidates(K) if not S else int(S)
    A, _ = candidates(idx, S, iteration, seed)
    new_i, new_d = np.empty((n, K), np.int32), np.empty((n, K))
    for r0 in range(0, n, chunk):
        a = A[r0:r0 + chunk]
        aa = np.where(a[:, :, None] >= 0, A[np.where(a >= 0, a, 0)], -1).reshape(a.shape[0], -1)
        new_i[r0:r0 + chunk], new_d[r0:r0 + chunk] = offer(X, K, np.concatenate([idx[r0:r0 + chunk], aa, a], 1), r0)
    changed = int(n * K - (new_i[:, :, None] == idx[:, None, :]).any(2).sum())
    return new_i, new_d, changed


def descent(X, K, n_projections=8, max_candidates=None, n_iters=12, delta=0.001, seed=10):
    """-> (idx, dist2, {"joins", "updates", "reason"}); reason 0: n_iters reached, 1: updates <= delta n K"""
    n = X.shape[0]
    idx, dist = start(X, K, n_projections, seed)
    info = {"joins": 0, "updates": 0, "reason": 0}
    for it in range(1, n_iters + 1):
        idx, dist, info["updates"] = join(X, idx, max_candidates, it, seed)
        info["joins"] = it
        if float(info["updates"]) <= delta * float(n * K):
            info["reason"] = 1
            break
    return idx, dist, info
