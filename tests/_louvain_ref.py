"""The Louvain specification of DESIGN.md §18 in numpy: integer weights, one synchronous round of local moving under the hashed
source / target bits, the fixed-order modularity, aggregation and the driver over the levels.  This is the project's own specification;
no parity with networkx, igraph or cuGraph is claimed.  Every sum of weights is an int64 sum (exact, order-independent), every fp64
expression is written in the operation order the kernels use, and the sum of the modularity's terms runs in the order of graph.hpp's
two-stage reduction, so the GPU tests ask for equal bits.  No Python loop runs over vertices or entries.  The case builders of the
tests are at the end."""
import numpy as np

from _umap_ref import GOLDEN, MASK, mix

QBITS = 24
MAX_FAILS, MAX_ROUNDS, MAX_LEVELS, TOL = 4, 200, 20, 1e-7


def _rows(rp):
    rp = np.asarray(rp, np.int64)
    return np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))


def _group_sum(key, w):
    """(unique keys ascending, int64 sum of w per key)"""
    if key.size == 0:
        return key.astype(np.int64), np.zeros(0, np.int64)
    o = np.argsort(key, kind="stable")
    ks, ws = key[o], np.asarray(w, np.int64)[o]
    st = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    return ks[st], np.add.reduceat(ws, st)


def _scatter_sum(idx, w, size):
    out = np.zeros(size, np.int64)
    u, s = _group_sum(np.asarray(idx, np.int64), w)
    out[u] = s
    return out


# ---- rule 1: integer weights ----------------------------------------------------------------------------------------------------------
def quantise(rp, col, val):
    """q = rint(val * 2^24 / wmax) per entry (zeros kept in place), the strengths k and 2m"""
    val = np.asarray(val, np.float64)
    wmax = val.max()
    q = np.rint(val * float(1 << QBITS) / wmax).astype(np.int64)
    k = _scatter_sum(_rows(rp), q, len(rp) - 1)
    return q, k, int(k.sum())


def drop_zeros(rp, col, q):
    """the CSR without its q = 0 entries"""
    keep = np.asarray(q) > 0
    row = _rows(rp)
    n = len(rp) - 1
    nrp = np.zeros(n + 1, np.int64)
    nrp[1:] = np.cumsum(np.bincount(row[keep], minlength=n))
    return nrp, np.asarray(col, np.int32)[keep], np.asarray(q, np.int64)[keep]


def strengths(rp, q):
    return _scatter_sum(_rows(rp), q, len(rp) - 1)


# ---- rule 2: one round ----------------------------------------------------------------------------------------------------------------
def round_key(seed, level, rnd):
    with np.errstate(over="ignore"):
        x0 = mix(np.uint64(((int(seed) & MASK) * GOLDEN + int(level)) & MASK))
        return mix(x0 + np.uint64(rnd))


def hbit(seed, level, rnd, c):
    """h(c): the top bit of mix(mix(mix(seed * GOLDEN + level) + round) + c)"""
    with np.errstate(over="ignore"):
        return (mix(round_key(seed, level, rnd) + np.asarray(c, np.uint64)) >> np.uint64(63)).astype(np.int64)


def move(rp, col, q, comm, gamma, seed, level, rnd, k=None, tot=None):
    """the proposals of one round from the state comm"""
    rp, col, q, comm = np.asarray(rp, np.int64), np.asarray(col, np.int64), np.asarray(q, np.int64), np.asarray(comm, np.int64)
    n = rp.size - 1
    row = _rows(rp)
    k = strengths(rp, q) if k is None else np.asarray(k, np.int64)
    tot = _scatter_sum(comm, k, n) if tot is None else np.asarray(tot, np.int64)
    m2 = float(int(k.sum()))
    off = col != row
    key, kin = _group_sum(row[off] * n + comm[col[off]], q[off])
    pr, pc = key // n, key % n
    c0 = comm[pr]
    own = pc == c0
    kin0 = np.zeros(n, np.int64)
    kin0[pr[own]] = kin[own]
    kf = k.astype(np.float64)
    stay = kin0.astype(np.float64) - ((gamma * kf) * (tot[comm] - k).astype(np.float64)) / m2
    gain = kin.astype(np.float64) - ((gamma * kf[pr]) * tot[pc].astype(np.float64)) / m2      # (own entries are not candidates)
    ok = ~own & (hbit(seed, level, rnd, c0) == 1) & (hbit(seed, level, rnd, pc) == 0)
    pr, pc, gain = pr[ok], pc[ok], gain[ok]
    o = np.lexsort((pc, -gain, pr))                        # per vertex: gain descending, then id ascending
    pr, pc, gain = pr[o], pc[o], gain[o]
    first = np.flatnonzero(np.r_[True, pr[1:] != pr[:-1]]) if pr.size else np.zeros(0, np.int64)
    bv, bc, bg = pr[first], pc[first], gain[first]
    go = bg > stay[bv]
    prop = comm.copy()
    prop[bv[go]] = bc[go]
    return prop.astype(np.int32)


# ---- rule 3: modularity ---------------------------------------------------------------------------------------------------------------
def fixed_sum(v):
    """graph.hpp's fixed_reduce: blocks of chunk values, 256 strided running sums per block folded by a tree, then the same once more"""
    def stage(v, chunk):
        n = v.size
        nb = (max(n, 1) + chunk - 1) // chunk
        R = (chunk + 255) // 256
        j, t = np.meshgrid(np.arange(R), np.arange(256), indexing="ij")
        loc = j * 256 + t
        idx = np.arange(nb)[:, None, None] * chunk + loc[None]
        ok = (loc[None] < chunk) & (idx < n)
        A = np.where(ok, v[np.minimum(idx, max(n - 1, 0))] if n else 0.0, 0.0)
        a = np.zeros((nb, 256))
        for jj in range(R):
            a = a + A[:, jj, :]
        w = 128
        while w > 0:
            a[:, :w] = a[:, :w] + a[:, w:2 * w]
            w >>= 1
        return a[:, 0].copy()
    v = np.asarray(v, np.float64)
    chunk = max(256, (v.size + 1023) // 1024)
    part = stage(v, chunk)
    return float(stage(part, part.size)[0])


def state(rp, col, q, comm, gamma, k=None):
    """(tot, in, the surviving ids ascending, Q) of a membership: Q = the fixed-order sum of the surviving communities' terms
    in / 2m - gamma * (t * t),  t = tot / 2m,  sorted by value: a function of the partition, not of its labels"""
    rp, col, q, comm = np.asarray(rp, np.int64), np.asarray(col, np.int64), np.asarray(q, np.int64), np.asarray(comm, np.int64)
    n = rp.size - 1
    row = _rows(rp)
    k = strengths(rp, q) if k is None else k
    m2 = float(int(k.sum()))
    tot = _scatter_sum(comm, k, n)
    inside = comm[row] == comm[col]
    inn = _scatter_sum(comm[row[inside]], q[inside], n)
    ids = np.flatnonzero(np.bincount(comm, minlength=n) > 0)
    t = tot[ids].astype(np.float64) / m2
    terms = inn[ids].astype(np.float64) / m2 - gamma * (t * t)
    return tot, inn, ids, fixed_sum(np.sort(terms))


def modularity_q(rp, col, q, membership, gamma=1.0):
    """Q of any integer labelling of an integer-weighted CSR (the labels are ranked first)"""
    comm = np.unique(np.asarray(membership), return_inverse=True)[1].reshape(-1)
    return state(rp, col, q, comm, gamma)[3]


def modularity(rp, col, val, membership, gamma=1.0):
    """the public modularity(): of a float-weighted symmetric CSR, after rule 1"""
    q = quantise(rp, col, val)[0]
    return modularity_q(rp, col, q, membership, gamma)


# ---- rule 4: aggregation --------------------------------------------------------------------------------------------------------------
def aggregate(rp, col, q, comm):
    """(row_ptr, col, q, new): the coarse CSR and new[c] = the coarse vertex of the surviving community c (-1 elsewhere)"""
    rp, col, q, comm = np.asarray(rp, np.int64), np.asarray(col, np.int64), np.asarray(q, np.int64), np.asarray(comm, np.int64)
    n = rp.size - 1
    ids = np.flatnonzero(np.bincount(comm, minlength=n) > 0)
    nc = ids.size
    new = np.full(n, -1, np.int64)
    new[ids] = np.arange(nc)
    row = _rows(rp)
    key, w = _group_sum(new[comm[row]] * nc + new[comm[col]], q)
    crp = np.zeros(nc + 1, np.int64)
    crp[1:] = np.cumsum(np.bincount(key // nc, minlength=nc))
    return crp, (key % nc).astype(np.int32), w, new


# ---- rule 5: the driver ---------------------------------------------------------------------------------------------------------------
def relabel_by_size(lab):
    """1 .. G by decreasing size, ties to the community with the smallest member"""
    lab = np.asarray(lab, np.int64)
    u, first, inv, cnt = np.unique(lab, return_index=True, return_inverse=True, return_counts=True)
    order = np.lexsort((first, -cnt))
    rank = np.empty(u.size, np.int64)
    rank[order] = np.arange(1, u.size + 1)
    return rank[inv.reshape(-1)].astype(np.int32)


def level(rp, col, q, gamma, seed, lev, tol=TOL, max_rounds=MAX_ROUNDS, max_fails=MAX_FAILS, trace=None):
    """one level from the singletons: (comm, rounds, Q); trace: a list that receives (round, accepted, Q of the round)"""
    n = len(rp) - 1
    k = strengths(rp, q)
    comm = np.arange(n, dtype=np.int32)
    tot, _, _, Q = state(rp, col, q, comm, gamma, k)
    rounds = fails = 0
    while rounds < max_rounds and fails < max_fails:
        prop = move(rp, col, q, comm, gamma, seed, lev, rounds, k, tot)
        rounds += 1
        tot2, _, _, Q2 = state(rp, col, q, prop, gamma, k)
        ok = Q2 > Q + tol
        if trace is not None:
            trace.append((rounds - 1, bool(ok), Q2))
        if ok:
            comm, tot, Q, fails = prop, tot2, Q2, 0
        else:
            fails += 1
    return comm, rounds, Q


def louvain_q(rp, col, q, gamma=1.0, seed=10, tol=TOL, max_levels=MAX_LEVELS, max_rounds=MAX_ROUNDS, max_fails=MAX_FAILS):
    """the driver on an integer-weighted CSR: {"membership" (1 .. G), "n_communities", "modularity", "levels": [{"n", "communities",
    "rounds", "modularity", "membership" (0-based coarse ids of the input's vertices)}]}.  A level that merges nothing is recorded and
    ends the run."""
    n0 = len(rp) - 1
    vmap = np.arange(n0, dtype=np.int64)
    levels = []
    for lev in range(max_levels):
        n = len(rp) - 1
        comm, rounds, Q = level(rp, col, q, gamma, seed, lev, tol, max_rounds, max_fails)
        crp, ccol, cq, new = aggregate(rp, col, q, comm)
        nc = len(crp) - 1
        vmap = new[np.asarray(comm, np.int64)[vmap]]
        levels.append({"n": n, "communities": nc, "rounds": rounds, "modularity": Q, "membership": vmap.astype(np.int32)})
        if nc == n:
            break
        rp, col, q = crp, ccol, cq
    return {"membership": relabel_by_size(vmap), "n_communities": int(levels[-1]["communities"]), "modularity": levels[-1]["modularity"],
            "levels": levels, "seed": seed}


def louvain(rp, col, val, gamma=1.0, seed=10, **kw):
    """the driver on a float-weighted symmetric CSR without diagonal entries (rules 1 - 5)"""
    q = quantise(rp, col, val)[0]
    return louvain_q(*drop_zeros(rp, col, q), gamma, seed, **kw)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
def csr_from_pairs(n, i, j, w, symmetric=True):
    """a CSR with sorted rows from entries (i, j, w); symmetric: the mirrored entries are added (i != j)"""
    i, j, w = np.asarray(i, np.int64), np.asarray(j, np.int64), np.asarray(w)
    if symmetric:
        d = i != j
        i, j, w = np.r_[i, j[d]], np.r_[j, i[d]], np.r_[w, w[d]]
    o = np.lexsort((j, i))
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(i, minlength=n))
    return rp, j[o].astype(np.int32), w[o]


def path(n=1025, dtype=np.float64):
    a = np.arange(n - 1)
    return csr_from_pairs(n, a, a + 1, np.ones(n - 1, dtype))


def ring_of_cliques(cliques=30, size=6, dtype=np.float64):
    n = cliques * size
    a, b = np.triu_indices(size, 1)
    i = (np.arange(cliques)[:, None] * size + a[None]).ravel()
    j = (np.arange(cliques)[:, None] * size + b[None]).ravel()
    ri = np.arange(cliques) * size + size - 1
    rj = (np.arange(cliques) + 1) % cliques * size
    i, j = np.r_[i, ri], np.r_[j, rj]
    return csr_from_pairs(n, i, j, np.ones(i.size, dtype))


def star(leaves=3000, dtype=np.float64):
    return csr_from_pairs(leaves + 1, np.zeros(leaves, np.int64), np.arange(1, leaves + 1), np.ones(leaves, dtype))


def complete_int(n=300, seed=3):
    """a complete graph with random integer weights and self-loops, as a coarse level has them"""
    rng = np.random.default_rng(seed)
    i, j = np.triu_indices(n, 0)
    return csr_from_pairs(n, i, j, rng.integers(1, 1 << 20, size=i.size).astype(np.int64))


def hub(length, extra=40, seed=4):
    """vertex 0 with exactly `length` entries, the other vertices in a ring with a few random chords: a row of a chosen length"""
    rng = np.random.default_rng(seed)
    n = length + 1 + extra
    i = np.r_[np.zeros(length, np.int64), np.arange(1, n - 1)]
    j = np.r_[np.arange(1, length + 1), np.arange(2, n)]
    w = rng.integers(1, 1000, size=i.size).astype(np.int64)
    return csr_from_pairs(n, i, j, w)


def hubs(n, count, seed=2, dtype=np.int64):
    """vertices 0 .. count - 1 adjacent to every vertex, the others in a ring: `count` rows of n - 1 entries; weights 1 .. 49 (as
    integers, or as floats divided by 49)"""
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(count), n)
    j = np.tile(np.arange(n), count)
    keep = i < j
    i, j = np.r_[i[keep], np.arange(count, n - 1)], np.r_[j[keep], np.arange(count + 1, n)]
    w = rng.integers(1, 50, size=i.size)
    return csr_from_pairs(n, i, j, w.astype(np.int64) if dtype == np.int64 else w / 49.0)


def planted(blocks=8, size=64, p_in=0.25, p_out=0.04, seed=7):
    """a noisy planted partition with random weights in (0, 1]: (rp, col, val, labels)"""
    rng = np.random.default_rng(seed)
    n = blocks * size
    lab = np.arange(n) // size
    i, j = np.triu_indices(n, 1)
    keep = rng.random(i.size) < np.where(lab[i] == lab[j], p_in, p_out)
    i, j = i[keep], j[keep]
    return csr_from_pairs(n, i, j, rng.uniform(0.05, 1.0, size=i.size)) + (lab,)


def knn_graph(X, K):
    """the fuzzy graph of the exact K-NN lists of X (§13's reference): (rp, col, val)"""
    import _umap_ref as U

    idx, d = U.knn_lists(X, K)
    return U.graph(idx, d)[:3]


def blobs_graph(n=1500, d=10, k=6, K=14, seed=0):
    import _umap_ref as U

    X, lab = U.blobs(n, d, k, seed)
    return knn_graph(X, K) + (lab, X)


def gaussian_graph(n=2000, d=50, K=14, seed=1):
    X = np.random.default_rng(seed).normal(size=(n, d))
    return knn_graph(X, K) + (X,)


def adjusted_rand(a, b):
    a = np.unique(a, return_inverse=True)[1].reshape(-1)
    b = np.unique(b, return_inverse=True)[1].reshape(-1)
    t = np.zeros((a.max() + 1, b.max() + 1), np.int64)
    np.add.at(t, (a, b), 1)
    c2 = lambda x: (x * (x - 1) // 2).sum()     # noqa: E731
    s, sa, sb, tot = c2(t), c2(t.sum(1)), c2(t.sum(0)), a.size * (a.size - 1) // 2
    e = sa * sb / tot
    return float((s - e) / (0.5 * (sa + sb) - e))
