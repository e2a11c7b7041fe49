"""The batch integration of DESIGN.md 23 restated in numpy, in fp64 or longdouble (dt).

It follows the specification step by step -- the hash, the working order, the start cells, the Lloyd rounds, the clustering rounds block
by block with the fold-the-others O tables, the closed-form ridge correction -- and takes every sum with numpy's own reductions in `dt`.
With dt = longdouble (64 bits of mantissa on x86) the sums that the GPU's are compared against carry 2^-11 of the GPU's rounding, which
is DESIGN.md 21's lesson: a reference in the precision of the code under test has an error of its own size.  cells = "working" takes
the sums over the cells in the working order instead of the stored one: the same numbers up to rounding, which is what the spread
between two stored orders measures.

The figures at the end were measured with this file (tests/test_harmony_cpu.py measures them again and compares)."""
import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
U = 2.0 ** -53


def mix64(z):
    """graph.hpp's mix64 on a Python integer"""
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def _mix64_np(z):
    z = z.copy()
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


def h(seed, s, n):
    """h(s, i) for i = 0 .. n - 1, as uint64"""
    base = np.uint64(mix64((seed * G + s) & M64))
    with np.errstate(over="ignore"):
        return _mix64_np(base + np.arange(n, dtype=np.uint64))


def blocks_of(seed, n, n_blocks):
    return (h(seed, 0, n) % np.uint64(n_blocks)).astype(np.int64)


def working_order(batch, seed, n_blocks):
    """the cells sorted by (block, batch, i)"""
    n = len(batch)
    return np.lexsort((np.arange(n), np.asarray(batch), blocks_of(seed, n, n_blocks)))


def start_cells(seed, n, K):
    """the K cells with the smallest h(1, i), ties to the lower i"""
    return np.lexsort((np.arange(n), h(seed, 1, n)))[:K]


def normalize(X, keep=None):
    """rows / their 2-norms; a zero row stays zero, or takes keep's row"""
    nrm = np.sqrt((X * X).sum(axis=1))
    out = X / np.where(nrm > 0, nrm, 1)[:, None]
    if keep is not None:
        out[nrm == 0] = keep[nrm == 0]
    return out


def assign(Zh, Y, batch=None, P=None, sigma=0.1, dt=np.longdouble):
    """R (n x K) of the assign pass; P: B x K or None"""
    Zh, Y = np.asarray(Zh, dt), np.asarray(Y, dt)
    D = 2 * (1 - Zh @ Y.T)
    R = np.exp(-(D - D.min(axis=1, keepdims=True)) / dt(sigma))
    if P is not None:
        R = R * np.asarray(P, dt)[np.asarray(batch)]
    return R / R.sum(axis=1, keepdims=True)


def cosines(Zh, Y, dt=np.longdouble):
    return np.asarray(Zh, dt) @ np.asarray(Y, dt).T


def sums(R, X, batch, B, seed, n_blocks, dt=np.longdouble):
    """(O[j, b, k], S[b, k, :], |.| sums of the same terms, the number of terms of each O and S entry)"""
    R, X, batch = np.asarray(R, dt), np.asarray(X, dt), np.asarray(batch)
    n, K = R.shape
    blk = blocks_of(seed, n, n_blocks)
    O, Oa, On = np.zeros((n_blocks, B, K), dt), np.zeros((n_blocks, B, K), dt), np.zeros((n_blocks, B), np.int64)
    S, Sa, Sn = np.zeros((B, K, X.shape[1]), dt), np.zeros((B, K, X.shape[1]), dt), np.zeros(B, np.int64)
    for b in range(B):
        ib = np.flatnonzero(batch == b)
        S[b], Sa[b], Sn[b] = R[ib].T @ X[ib], np.abs(R[ib]).T @ np.abs(X[ib]), ib.size
        for j in range(n_blocks):
            ij = ib[blk[ib] == j]
            O[j, b], Oa[j, b], On[j, b] = R[ij].sum(axis=0), np.abs(R[ij]).sum(axis=0), ij.size
    return O, S, Oa, Sa, On, Sn


def ridge(N, S, lam):
    """W[b, k, :] from N[b, k] and S[b, k, :]: the closed form of step 5"""
    dt = S.dtype.type
    q = N / (N + dt(lam))
    s = dt(lam) * q.sum(axis=0)                                     # K
    num = S.sum(axis=0) - (q[:, :, None] * S).sum(axis=0)           # K x d
    ok = s > 0
    w0 = np.where(ok[:, None], num / np.where(ok, s, 1)[:, None], 0)
    W = (S - N[:, :, None] * w0[None]) / (N + dt(lam))[:, :, None]
    W[:, ~ok] = 0
    return W


def ridge_solve(N, S, lam):
    """the same W from numpy.linalg.solve on the (B + 1) x (B + 1) system of every cluster (fp64)"""
    B, K, d = S.shape
    W = np.zeros((B, K, d))
    for k in range(K):
        A = np.zeros((B + 1, B + 1))
        A[0, 0] = N[:, k].sum()
        A[0, 1:] = A[1:, 0] = N[:, k]
        A[1:, 1:] = np.diag(N[:, k] + lam)
        rhs = np.vstack([S[:, k].sum(axis=0)[None], S[:, k]])
        W[:, k] = np.linalg.solve(A, rhs)[1:]
    return W


def correct(Z, R, batch, W, dt=np.longdouble):
    Z, R, W = np.asarray(Z, dt), np.asarray(R, dt), np.asarray(W, dt)
    return Z - np.einsum("ik,ikc->ic", R, W[np.asarray(batch)])


def correct_abs(Z, R, batch, W):
    return np.abs(Z) + np.einsum("ik,ikc->ic", np.abs(R), np.abs(W[np.asarray(batch)]))


def harmony(Z, batch, n_clusters=None, sigma=0.1, theta=2.0, lam=1.0, max_iter=10, max_iter_cluster=20, n_blocks=20,
            epsilon_cluster=1e-5, epsilon_harmony=1e-4, init_iter=10, seed=1, dt=np.float64, cells="stored"):
    """the whole call.  Beyond the library's result: "margins" (every stop decision's |obj_(r-1) - obj_r - eps |obj_(r-1)||, clustering and
    outer), "cos_gap" (the smallest gap between the best and the second cosine of a cell, per start round; "cos_gap_positive": exact ties, which
    identical centroids give on any hardware, left out), "start_empty" (the clusters
    without a cell, per start round) and "all_objectives"."""
    levels, batch = np.unique(np.asarray(batch), return_inverse=True)
    batch = batch.reshape(-1)
    n, d = Z.shape
    B = levels.size
    K = min(int(round(n / 30)), 100) if n_clusters is None else int(n_clusters)
    perm = working_order(batch, seed, n_blocks) if cells == "working" else np.arange(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    # everything below is held in `perm` order; idx[j]: the positions of block j's cells
    Z0 = np.asarray(Z, dt)[perm]
    bt = batch[perm]
    blk = blocks_of(seed, n, n_blocks)[perm]
    idx = [np.flatnonzero(blk == j) for j in range(n_blocks)]
    Phi = np.zeros((n, B), dt)
    Phi[np.arange(n), bt] = 1
    Pr = (Phi.sum(axis=0) / dt(n))
    sig, th = dt(sigma), dt(theta)
    Zh = normalize(Z0)
    Y = Zh[inv[start_cells(seed, n, K)]].copy()
    gaps, gaps_pos, empty = [], [], []
    for _ in range(init_iter):
        cs = Zh @ Y.T
        a = cs.argmax(axis=1)
        top = np.sort(cs, axis=1)
        gap = top[:, -1] - top[:, -2]
        gaps.append(float(gap.min()))
        gaps_pos.append(float(gap[gap > 0].min()))
        A = np.zeros((n, K), dt)
        A[np.arange(n), a] = 1
        empty.append(int((A.sum(axis=0) == 0).sum()))
        Y = normalize(A.T @ Zh, keep=Y)

    def dist():
        return 2 * (1 - Zh @ Y.T)

    D = dist()
    R = np.exp(-(D - D.min(axis=1, keepdims=True)) / sig)
    R /= R.sum(axis=1, keepdims=True)
    Oj = np.stack([R[idx[j]].T @ Phi[idx[j]] for j in range(n_blocks)])          # n_blocks x K x B
    objective, rounds, margins, allobj = [], [], [], []
    converged = False
    Zc = Z0
    for t in range(max_iter):
        obj = []
        for r in range(1, max_iter_cluster + 1):
            Y = normalize(R.T @ Zh, keep=Y)
            D = dist()
            for j in range(n_blocks):
                ij = idx[j]
                if ij.size == 0:
                    continue
                O = np.zeros((K, B), dt)
                for j2 in range(n_blocks):
                    if j2 != j:
                        O = O + Oj[j2]
                E = O.sum(axis=1, keepdims=True) * Pr[None]
                P = ((E + 1) / (O + 1)) ** th
                Rj = np.exp(-(D[ij] - D[ij].min(axis=1, keepdims=True)) / sig) * P[:, bt[ij]].T
                R[ij] = Rj / Rj.sum(axis=1, keepdims=True)
                Oj[j] = R[ij].T @ Phi[ij]
            O = np.zeros((K, B), dt)
            for j2 in range(n_blocks):
                O = O + Oj[j2]
            E = O.sum(axis=1, keepdims=True) * Pr[None]
            with np.errstate(divide="ignore", invalid="ignore"):
                mid = np.where(R > 0, sig * np.log(np.where(R > 0, R, 1)), 0)
            pen = sig * th * np.log((O + 1) / (E + 1))
            obj.append((R * (D + mid + pen[:, bt].T)).sum())
            if r >= 2 and epsilon_cluster > 0:
                margins.append(float(abs(obj[-2] - obj[-1] - dt(epsilon_cluster) * abs(obj[-2]))))
                if obj[-2] - obj[-1] < dt(epsilon_cluster) * abs(obj[-2]):
                    break
        rounds.append(len(obj))
        objective.append(obj[-1])
        allobj.extend(obj)
        N = O.T.copy()                                               # B x K
        S = np.stack([(R * Phi[:, b:b + 1]).T @ Z0 for b in range(B)])               # B x K x d
        W = ridge(N, S, lam)
        Zc = Z0 - np.einsum("ik,ikc->ic", R, W[bt])
        Zh = normalize(Zc)
        if t >= 1 and epsilon_harmony > 0:
            margins.append(float(abs(objective[-2] - objective[-1] - dt(epsilon_harmony) * abs(objective[-2]))))
            if objective[-2] - objective[-1] < dt(epsilon_harmony) * abs(objective[-2]):
                converged = True
                break
    return {"Z_corr": Zc[inv], "Y": Y, "R": R[inv], "objective": np.array(objective), "rounds": np.array(rounds), "n_iter": len(objective),
            "converged": converged, "n_clusters": K, "n_batches": B, "batch_levels": levels, "margins": margins, "cos_gap": gaps, "cos_gap_positive": gaps_pos, "start_empty": empty,
            "all_objectives": np.array(allobj)}


def planted(n, seed=0):
    """(Z n x 10, batch, label): six clusters, three batches, two of the clusters missing from or rare in a batch, batch offsets"""
    rng = np.random.default_rng(seed)
    d, nc, nb = 10, 6, 3
    centres = 6.0 * np.eye(nc, d) + 0.5 * rng.standard_normal((nc, d))
    label = rng.integers(0, nc, n)
    batch = rng.integers(0, nb, n)
    move = np.flatnonzero((label == 5) & (batch == 0))
    batch[move] = rng.integers(1, nb, move.size)
    cand = np.flatnonzero((label == 0) & (batch == 1))
    batch[cand[rng.random(cand.size) < 0.8]] = 0
    off = rng.standard_normal((nb, d))
    off = 2.0 * off / np.sqrt((off * off).sum(axis=1, keepdims=True))
    Z = centres[label] + off[batch] + rng.standard_normal((n, d))
    return np.ascontiguousarray(Z), batch.astype(np.int64), label.astype(np.int64)


def neighbour_shares(Z, batch, label, k=30):
    """(the mean share of a cell's k nearest neighbours in its own batch, the same for its label, the smallest per-label mean of the latter)"""
    Z = np.asarray(Z, np.float64)
    sq = (Z * Z).sum(axis=1)
    D = sq[:, None] + sq[None] - 2 * Z @ Z.T
    np.fill_diagonal(D, np.inf)
    nn = np.argpartition(D, k, axis=1)[:, :k]
    same_b = (batch[nn] == batch[:, None]).mean(axis=1)
    same_l = (label[nn] == label[:, None]).mean(axis=1)
    return float(same_b.mean()), float(same_l.mean()), float(min(same_l[label == c].mean() for c in np.unique(label)))


def spread(a, b, relative=False):
    """max |a - b| in fp64, relative to max |b| when asked"""
    e = float(np.abs(np.asarray(a, np.longdouble) - np.asarray(b, np.longdouble)).max())
    return e / float(np.abs(b).max()) if relative else e


# ---- the whole-call inputs of the GPU tests and the figures measured on them ---------------------------------------------------------------
WHOLE = (1500, 1025)                                         # planted(n), seed 0
FIXED = dict(max_iter=5, max_iter_cluster=10, epsilon_cluster=0.0, epsilon_harmony=0.0)
SEEDS = (1, 2, 3, 4, 5)
# The rounding spread of this reference as measured, rounded up to two digits: the larger of fp64 against longdouble with the cells summed
# in the stored order and in the working order; "Z_corr" relative to max |Z_corr|, "Y" and "R" absolute (FIXED counts, seed 1);
# "objective" absolute over every round of the default call (seed 1).  tests/test_harmony_cpu.py measures them again and accepts the
# record only while it lies between the measured figure and 1.25 x it.
SPREAD = {1500: {"Z_corr": 1.2e-15, "Y": 7.5e-16, "R": 1.7e-15, "objective": 2.6e-13},
          1025: {"Z_corr": 1.7e-15, "Y": 8.5e-16, "R": 3.5e-15, "objective": 8.3e-14}}
# The default call (seed 1): what the library has to decide as well.
DECISIONS = {1500: {"n_iter": 3, "rounds": (20, 10, 2), "converged": True}, 1025: {"n_iter": 3, "rounds": (18, 3, 2), "converged": True}}
# The neighbour shares (k = 30) of the default call over SEEDS: before, the worst of the five after (the highest same-batch share, the
# lowest same-label share) and the seed-to-seed spread (max - min) of each.  Chance for the same-batch share is 0.336 / 0.337.
QUALITY = {1500: {"before": (0.6723, 0.9983), "same_batch_worst": 0.38160, "same_batch_spread": 0.00100, "same_label_worst": 0.99976,
                  "same_label_spread": 0.00003, "min_cluster_label": 0.9990},
           1025: {"before": (0.6523, 0.9986), "same_batch_worst": 0.36944, "same_batch_spread": 0.00222, "same_label_worst": 0.99954,
                  "same_label_spread": 0.00030, "min_cluster_label": 0.9988}}
