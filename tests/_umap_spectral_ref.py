"""The spectral start of DESIGN.md §15 in numpy fp64: the seeded inputs, the connected components (union-find), the operator
M = D^-1/2 W D^-1/2 and its dense eigenpairs, the sign rule, the Davis-Kahan vector bound, and an emulation of the Lanczos recurrence
with full reorthogonalisation.  This is the project's own specification (modelled on uwot's "normlaplacian" start); it claims no bit
parity with uwot or umap-learn.  The GPU tests compare libsharp_hip.so with these functions; tests/test_umap_spectral_cpu.py asserts
the premises those comparisons rely on."""
import functools

import numpy as np

import _umap_ref as ref

EPS = 2.0 ** -52
TOL = 1e-10                                      # the solver tests' tolerance
MAX_STEPS = 400


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _box(n, sides, seed, d=10):
    """n points uniform in a box with the given sides, embedded in d dimensions with N(0, 0.02^2) noise.  Unequal sides keep the
    Laplacian's bottom eigenvalues apart."""
    rng = np.random.default_rng(seed)
    X = rng.normal(0.0, 0.02, size=(n, d))
    X[:, :len(sides)] += rng.uniform(0.0, 1.0, size=(n, len(sides))) * np.asarray(sides)
    return X


def slab(n=1025, seed=15):
    return _box(n, (4.0, 1.7, 0.7), seed)


def ribbon(n=257, seed=15):
    return _box(n, (4.0, 1.0), seed)


def two_slabs(n=1025):
    """two slabs 100 apart"""
    a, b = slab(n // 2, 16), slab(n - n // 2, 17)
    b[:, 0] += 100.0
    return np.vstack([a, b])


@functools.lru_cache(maxsize=None)
def lists(name, K):
    X = {"slab": slab, "ribbon": ribbon, "two_slabs": two_slabs, "blobs": lambda: ref.blobs()[0]}[name]()
    idx, d = ref.knn_lists(X, K)
    return idx.astype(np.int32), d


def with_hub(rp, col, val, degree=688, weight=0.25, seed=3):
    """vertex 0 joined, both ways with the given weight, to seeded vertices it is not joined to yet, until its row holds `degree`
    entries: a hub row that needs several passes of 64 lanes"""
    n = rp.size - 1
    W = np.zeros((n, n))
    row = np.repeat(np.arange(n), np.diff(rp))
    W[row, col] = val
    free = np.setdiff1d(np.arange(1, n), col[rp[0]:rp[1]])
    add = np.random.default_rng(seed).choice(free, degree - int(rp[1] - rp[0]), replace=False)
    W[0, add] = weight
    W[add, 0] = weight
    return csr_of(W)


def csr_of(W):
    n = W.shape[0]
    r, c = np.nonzero(W)
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, r + 1, 1)
    return np.cumsum(rp), c.astype(np.int32), W[r, c].copy()


def path_graph(n=1025, seed=4):
    """the path on n vertices numbered by a seeded permutation, unit weights"""
    perm = np.random.default_rng(seed).permutation(n)
    W = np.zeros((n, n))
    W[perm[:-1], perm[1:]] = 1.0
    W[perm[1:], perm[:-1]] = 1.0
    return csr_of(W)


def edges_and_triangle():
    """512 disjoint edges plus a triangle on shuffled numbers: n = 1 027, 513 components"""
    n = 1027
    perm = np.random.default_rng(6).permutation(n)
    W = np.zeros((n, n))
    a, b = perm[0:1024:2], perm[1:1024:2]
    W[a, b] = W[b, a] = 1.0
    t = perm[1024:]
    for x, y in ((0, 1), (1, 2), (0, 2)):
        W[t[x], t[y]] = W[t[y], t[x]] = 1.0
    return csr_of(W)


@functools.lru_cache(maxsize=None)
def case(name):
    """the solver's inputs as (row_ptr, col, val): slab14, slab64, hub, ribbon, and the inputs of the other outcomes: two_slabs, blobs,
    path"""
    if name == "hub":
        return with_hub(*case("slab14"))
    if name == "path":
        return path_graph()
    src, K = {"slab14": ("slab", 14), "slab64": ("slab", 64), "ribbon": ("ribbon", 14), "two_slabs": ("two_slabs", 14),
              "blobs": ("blobs", 14)}[name]
    return ref.graph(*lists(src, K))[:3]


SOLVER_CASES = ("slab14", "slab64", "hub", "ribbon")


# ---- components -----------------------------------------------------------------------------------------------------------------------
def components(rp, col):
    """label[i] = the smallest vertex of i's component (union-find over the pattern, an edge in both directions), and their number"""
    n = rp.size - 1
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    row = np.repeat(np.arange(n), np.diff(rp))
    for i, j in zip(row, col):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    label = np.array([find(i) for i in range(n)], np.int32)
    return label, int((label == np.arange(n)).sum())


# ---- the operator and its dense eigenpairs ----------------------------------------------------------------------------------------------
def operator(rp, col, val):
    """M = D^-1/2 W D^-1/2 (dense) and q0 = sqrt(deg) / ||sqrt(deg)||"""
    n = rp.size - 1
    row = np.repeat(np.arange(n), np.diff(rp))
    W = np.zeros((n, n))
    W[row, col] = val
    deg = W.sum(1)
    s = 1.0 / np.sqrt(deg)
    M = W * np.outer(s, s)                       # (symmetric to the bit where W is)
    q0 = np.sqrt(deg)
    return M, q0 / np.linalg.norm(q0)


def sign_rule(V):
    """each column's largest |component| made positive, ties to the lowest index"""
    V = np.asarray(V, np.float64)
    arg = np.abs(V).argmax(0)
    return V * np.where(V[arg, np.arange(V.shape[1])] < 0, -1.0, 1.0)


@functools.lru_cache(maxsize=None)
def dense(name):
    """(M, q0, lam, U, gap): lam the three largest eigenvalues of M below the trivial one (descending), U their unit vectors under
    the sign rule, gap_j the distance from lam_j to its nearest other eigenvalue"""
    M, q0 = operator(*case(name))
    w, Q = np.linalg.eigh(M)
    w, Q = w[::-1], Q[:, ::-1]
    lam, U = w[1:4], sign_rule(Q[:, 1:4])
    gap = np.array([min(w[j] - w[j + 1], w[j - 1] - w[j]) for j in (1, 2, 3)])
    return M, q0, lam, U, gap


def vector_bound(r, gap, n):
    """Davis-Kahan: a unit vector with residual r against a symmetric matrix lies within sqrt(2) (r + n eps) / gap of the unit
    eigenvector (n eps for eigh's own error)"""
    return np.sqrt(2.0) * (np.asarray(r) + n * EPS) / np.asarray(gap)


def sign_margin(U):
    """per column: the largest |component| minus the largest of the opposite sign"""
    U = np.asarray(U)
    return np.array([U[:, j].max() - max(-U[:, j].min(), 0.0) for j in range(U.shape[1])])


# ---- the solver, emulated -------------------------------------------------------------------------------------------------------------
def start_vector(n):
    with np.errstate(over="ignore"):
        x = ref.mix(np.uint64(ref.GOLDEN) + np.arange(n, dtype=np.uint64))
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5


def lanczos(M, q0, dims, tol=TOL, max_steps=MAX_STEPS, check_every=8):
    """§15's recurrence: {"outcome", "steps", "theta", "V", "residual"}; the estimates when it does not converge"""
    n = M.shape[0]
    max_steps = min(max_steps, n - 2)
    Q = np.zeros((n, max_steps + 2))
    Q[:, 0] = q0

    def extend(u, k):
        for _ in range(2):
            u = u - Q[:, :k] @ (Q[:, :k].T @ u)
        b = np.linalg.norm(u)
        Q[:, k] = u / b
        return b

    extend(start_vector(n), 1)
    alpha, beta, est = [], [], None
    for k in range(1, max_steps + 1):
        u = M @ Q[:, k]
        alpha.append(Q[:, k] @ u)
        beta.append(extend(u, k + 1))
        if k % check_every and k != max_steps:
            continue
        if k < dims:
            continue
        T = np.diag(alpha) + np.diag(beta[:-1], 1) + np.diag(beta[:-1], -1)
        w, S = np.linalg.eigh(T)
        top = np.argsort(-w, kind="stable")[:dims]
        est = np.abs(beta[-1] * S[-1, top])
        if (est <= tol).all():
            V = Q[:, 1:k + 1] @ S[:, top]
            V = V / np.linalg.norm(V, axis=0)
            r = np.linalg.norm(M @ V - V * w[top], axis=0)
            if (r <= tol).all():
                return {"outcome": 0, "steps": k, "theta": w[top], "V": sign_rule(V), "residual": r}
    return {"outcome": 2, "steps": max_steps, "theta": None, "V": None, "residual": est}
