"""Diffusion maps and diffusion pseudotime of DESIGN.md §26 in numpy fp64: the transition operator T and its scaling a, the chosen
connected component (union-find, the tie rule) as a CSR of its own, the dense eigenpairs under the sign rule with their gaps, the
pseudotime formula, and an emulation of the thick-restart Lanczos recurrence with the library's constants.  This is the project's own
specification (modelled on scanpy's tl.diffmap / tl.dpt and Haghverdi et al. 2016); it claims no parity with scanpy or destiny.  The
inputs are tests/_umap_spectral_ref.py's.  The GPU tests compare libsharp_hip.so with these functions; tests/test_diffmap_cpu.py asserts
the premises those comparisons rely on."""
import functools

import numpy as np

import _umap_spectral_ref as sref

EPS = sref.EPS
TOL = 1e-10                                      # the solver tests' tolerance
MAX_MATVECS = 4000                               # kDiffmapMaxMatvecs
CHECK_EVERY = 8                                  # kDiffmapCheckEvery


def keep(k):
    """the columns a restart keeps for k wanted pairs (diffmap_keep)"""
    return 8 * ((k + k // 2 + 1 + 7) // 8)


def basis(k):
    """the basis' capacity (diffmap_basis)"""
    return 2 * keep(k) + 16


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def small_graph(n=20, seed=8):
    """a connected graph on n vertices: a ring with seeded weights in [0.5, 1.5) plus five chords"""
    rng = np.random.default_rng(seed)
    W = np.zeros((n, n))
    for i in range(n):
        j = (i + 1) % n
        W[i, j] = W[j, i] = rng.uniform(0.5, 1.5)
    for _ in range(5):
        i, j = rng.choice(n, 2, replace=False)
        W[i, j] = W[j, i] = rng.uniform(0.5, 1.5)
    return sref.csr_of(W)


def two_halves(n=40, seed=9):
    """two rings of n / 2 vertices each, on interleaved numbers (even / odd): two components of one size"""
    rng = np.random.default_rng(seed)
    W = np.zeros((n, n))
    for part in (np.arange(1, n, 2), np.arange(0, n, 2)):
        for a, b in zip(part, np.roll(part, -1)):
            W[a, b] = W[b, a] = rng.uniform(0.5, 1.5)
    return sref.csr_of(W)


def with_empty_row(rp, col, val, at=5):
    """the CSR with vertex `at` cut off: its row emptied and its column removed"""
    W = dense_w(rp, col, val)
    W[at, :] = 0.0
    W[:, at] = 0.0
    return sref.csr_of(W)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "small":
        return small_graph()
    if name == "slab_odd":                       # n = 1 023 = 3 * 11 * 31: no multiple of 4, 64 or 256
        idx, d = sref.ref.knn_lists(sref.slab(1023, 21), 14)
        return sref.ref.graph(idx.astype(np.int32), d)[:3]
    return sref.case(name)


# (name, n_comps): the solver's cases at tol 1e-10
SOLVER_CASES = (("slab14", 2), ("slab14", 4), ("slab14", 10), ("slab14", 16), ("slab14", 32), ("slab64", 16), ("hub", 16), ("ribbon", 16),
                ("small", 4))
RESTART_CASE = ("slab14", 16)                    # the emulation restarts at least twice here
PATH_CAP = 300                                   # operator applications the path graph is given in the not-converged test (n_comps 16)


def dense_w(rp, col, val):
    n = rp.size - 1
    W = np.zeros((n, n))
    W[np.repeat(np.arange(n), np.diff(rp)), col] = val
    return W


# ---- the operator ---------------------------------------------------------------------------------------------------------------------
def transitions(rp, col, val, density=True, dtype=np.float64):
    """(a, z): q_i = sum_j W_ij; density: z_i = (1 / q_i) sum_j W_ij / q_j, a_i = 1 / (q_i sqrt(z_i)); else z = q, a = 1 / sqrt(q).
    An empty row: a = z = 0.  dtype np.longdouble gives the reference the GPU's sums are compared with."""
    W = dense_w(rp, col, val).astype(dtype)
    q = W.sum(1)
    live = q > 0
    qs = np.where(live, q, 1)
    if density:
        z = (W / qs[None, :]).sum(1) / qs
        a = 1 / (qs * np.sqrt(np.where(live, z, 1)))
    else:
        z = q.copy()
        a = 1 / np.sqrt(qs)
    return np.where(live, a, 0), np.where(live, z, 0)


def operator(rp, col, val, density=True):
    """(T, q0): T = W o (a a^T) dense (symmetric to the bit where W is) and q0 = sqrt(z) / ||sqrt(z)||.  Without density normalisation a
    is computed as _umap_spectral_ref.operator computes its s, so T equals its M bit for bit."""
    W = dense_w(rp, col, val)
    if density:
        a, z = transitions(rp, col, val, True)
    else:
        z = W.sum(1)
        a = 1.0 / np.sqrt(z)
    T = W * np.outer(a, a)
    q0 = np.sqrt(z)
    return T, q0 / np.linalg.norm(q0)


# ---- the component --------------------------------------------------------------------------------------------------------------------
def component(rp, col, val, root=-1):
    """(label, count, (sub_rp, sub_col, sub_val), new_id): root's component, or the largest with ties to the smallest label; its rows and
    columns renumbered in ascending order of the old ids; new_id = -1 outside"""
    lab, count = sref.components(rp, col)
    n = rp.size - 1
    if root >= 0:
        chosen = int(lab[root])
    else:
        size = np.bincount(lab, minlength=n)
        chosen = int(np.argmax(size))            # (the first maximum: the smallest label)
    inside = lab == chosen
    new_id = np.where(inside, np.cumsum(inside) - 1, -1).astype(np.int32)
    row = np.repeat(np.arange(n), np.diff(rp))
    e = inside[row]
    sub_rp = np.concatenate([[0], np.cumsum(np.diff(rp)[inside])]).astype(np.int64)
    return chosen, count, (sub_rp, new_id[col[e]].astype(np.int32), val[e].copy()), new_id


# ---- the dense eigenpairs -------------------------------------------------------------------------------------------------------------
def dense_of(T, n_comps):
    """(lam, U, gap) of a dense symmetric T: lam its n_comps largest eigenvalues, descending (lam[0] is the trivial 1 as eigh gives it), U
    their unit vectors under the sign rule, gap_j (j >= 1) the distance from lam_j to its nearest other eigenvalue (gap[0] = lam_0 - lam_1)"""
    w, Q = np.linalg.eigh(T)
    w, Q = w[::-1], Q[:, ::-1]
    return _top(w, Q, n_comps)


def _top(w, Q, n_comps):
    lam, U = w[:n_comps].copy(), sref.sign_rule(Q[:, :n_comps])
    gap = np.array([w[0] - w[1]] + [min(w[j] - w[j + 1], w[j - 1] - w[j]) for j in range(1, n_comps)])
    return lam, U, gap


@functools.lru_cache(maxsize=None)
def _eigh(name, density):
    T, q0 = operator(*case(name), density)
    w, Q = np.linalg.eigh(T)
    return T, q0, w[::-1], Q[:, ::-1]


def dense(name, n_comps, density=True):
    """(T, q0, lam, U, gap) of a named case: dense_of's pairs of its T (one eigh per case, shared by the tests)"""
    T, q0, w, Q = _eigh(name, density)
    return (T, q0) + _top(w, Q, n_comps)


# ---- pseudotime -----------------------------------------------------------------------------------------------------------------------
def dpt(evals, evecs, roots, n_dcs=10, normalize=True):
    """out[i, r] = sqrt(sum_{l=1}^{n_dcs-1} (w_l (psi_l(root_r) - psi_l(i)))^2), w = lambda / (1 - lambda), l ascending; inf for a row of
    NaN; normalize: each column divided by its largest finite value"""
    evals, evecs = np.asarray(evals, np.float64), np.asarray(evecs, np.float64)
    roots = np.atleast_1d(roots)
    w = evals / (1.0 - np.where(evals == 1.0, 0.0, evals))
    out = np.zeros((evecs.shape[0], roots.size))
    with np.errstate(invalid="ignore"):
        for l in range(1, n_dcs):
            t = w[l] * (evecs[roots, l][None, :] - evecs[:, l][:, None])
            out += t * t
        out = np.sqrt(out)
    out[np.isnan(evecs[:, 0])] = np.inf
    if normalize:
        for r in range(roots.size):
            fin = np.isfinite(out[:, r])
            mx = out[fin, r].max()
            if mx > 0:
                out[fin, r] = out[fin, r] / mx
    return out


# ---- the solver, emulated -------------------------------------------------------------------------------------------------------------
def thick_restart(T, q0, k, tol=TOL, cap=MAX_MATVECS, m=None, p=None, check_every=CHECK_EVERY):
    """diffmap_solve's recurrence: {"outcome", "steps", "restarts", "theta", "V", "residual"} (V: n x k unit Ritz vectors under the sign
    rule, residual their true residuals)"""
    n = T.shape[0]
    p = keep(k) if p is None else p
    m = min(basis(k) if m is None else m, n - 1)
    Q = np.zeros((n, m + 2))
    Q[:, 0] = q0
    u = sref.start_vector(n)
    for _ in range(2):
        u = u - q0 * (q0 @ u)
    Q[:, 1] = u / np.linalg.norm(u)
    H, beta = np.zeros((m, m)), np.zeros(m + 1)
    jc = jr = steps = restarts = 0
    while True:
        nc = jc + 2
        u = T @ Q[:, jc + 1]
        c = Q[:, :nc].T @ u
        H[:jc + 1, jc] = c[1:]
        H[jc, :jc + 1] = c[1:]
        u = u - Q[:, :nc] @ c
        u = u - Q[:, :nc] @ (Q[:, :nc].T @ u)
        b = np.linalg.norm(u)
        beta[jc] = b
        Q[:, jc + 2] = u / b if b > 0 else 0.0
        jc += 1
        steps += 1
        full, capped = jc == m, steps >= cap
        if steps % check_every and not full and not capped:
            continue
        jj, exhausted = jc, False
        for t in range(jr, jc):
            if not beta[t] > 64 * EPS:
                jj, exhausted = t + 1, True
                break
        if jj >= n - 1:
            exhausted = True
        if jj < k:
            if exhausted or capped:
                raise RuntimeError("fewer than k pairs")
            continue
        w, S = np.linalg.eigh(H[:jj, :jj])
        w, S = w[::-1], S[:, ::-1]
        est = np.zeros(k) if exhausted else np.abs(beta[jj - 1] * S[jj - 1, :k])
        conv = bool((est <= tol).all())
        if not conv and not capped and not full:
            continue
        kp = max(k, min(p, jj - 1))
        Y = Q[:, 1:jj + 1] @ S[:, :kp]
        nxt = Q[:, jj + 1].copy()
        Q[:, 1:kp + 1] = Y
        if kp < jj:
            Q[:, kp + 1] = nxt
        H[:] = 0.0
        H[np.arange(kp), np.arange(kp)] = w[:kp]
        jc = jr = kp
        if conv or capped:
            V = Y[:, :k] / np.linalg.norm(Y[:, :k], axis=0)
            r = np.linalg.norm(T @ V - V * w[:k], axis=0)
            ok = bool((r <= tol).all())
            if ok or capped or exhausted:
                return {"outcome": 0 if ok else 2, "steps": steps, "restarts": restarts, "theta": w[:k].copy(), "V": sref.sign_rule(V),
                        "residual": r}
        restarts += 1


@functools.lru_cache(maxsize=None)
def emulated(name, n_comps, density=True, cap=MAX_MATVECS):
    T, q0 = operator(*case(name), density)
    return thick_restart(T, q0, n_comps - 1, cap=cap)
