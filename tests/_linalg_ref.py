"""Plain numpy restatements of what sharp_amd/csrc/linalg.hip computes (linalg.hpp states each operation), and the seeded inputs of the
linalg tests.  Test infrastructure: tests/test_linalg_cpu.py pins every function here, tests/test_linalg_gpu.py compares the kernels
with them.

Precision: integer operands are multiplied in int64 (exact), everything else in np.longdouble (64-bit mantissa on x86: 2^-11 of an fp64
rounding per operation).  Two results are single IEEE operations on fp64 inputs and are therefore restated IN fp64, where the one
rounding is the kernel's own: the squares of nn_ref and the `1 - S` of row_prep_ref's D (a longdouble result rounded to fp64 afterwards
could round twice)."""
import numpy as np

EPS53 = 2.0 ** -53
NN_INF = 1.0e300                                   # linalg.hip NN_INF / hclust_task.hpp HC_INF
SENTINEL_BITS = np.uint64(0x7FF8C0DE5EED0001)      # include/sharp_hip.h: what the batch test entries pre-fill their outputs with


def rup(v, m):
    return (v + m - 1) // m * m


# ---- the GEMM ---------------------------------------------------------------------------------------------------------------------------
def gemm_ref(At, Bt, epilogue=0):
    """C = At^T Bt for k-major operands At (K x M), Bt (K x N).  Integer arrays: the int64 product (epilogue 0 only).  Otherwise the
    np.longdouble product with linalg.hpp's epilogues: 0 = v; 1 = 1 - clamp(v, -1, 1) with a zero diagonal; 2 = clamp(v) with a unit
    diagonal (the diagonal is row == col, also of a matrix that is not square)."""
    At, Bt = np.asarray(At), np.asarray(Bt)
    assert At.ndim == 2 and Bt.ndim == 2 and At.shape[0] == Bt.shape[0]
    if np.issubdtype(At.dtype, np.integer) and np.issubdtype(Bt.dtype, np.integer):
        assert epilogue == 0
        return At.astype(np.int64).T @ Bt.astype(np.int64)
    v = At.astype(np.longdouble).T @ Bt.astype(np.longdouble)
    if epilogue == 0:
        return v
    assert epilogue in (1, 2)
    v = np.clip(v, np.longdouble(-1), np.longdouble(1))
    d = np.arange(min(v.shape))
    if epilogue == 1:
        v = np.longdouble(1) - v
        v[d, d] = 0
    else:
        v[d, d] = 1
    return v


def gemm_bound(At, Bt):
    """|fl(sum_k a_k b_k) - sum_k a_k b_k| <= g_K sum_k |a_k b_k|, g_K = K u / (1 - K u), u = 2^-53: K products and K - 1 additions in
    any order, fused or not (Higham, Accuracy and Stability of Numerical Algorithms, (3.5) and section 3.1's remark on the order)."""
    K = At.shape[0]
    g = np.longdouble(K * EPS53) / (1 - np.longdouble(K * EPS53))
    return g * (np.abs(At).astype(np.longdouble).T @ np.abs(Bt).astype(np.longdouble))


def nn_ref(Cmat, n, square):
    """GemmTask::nn of the n x n matrix in Cmat[:n, :n] (fp64): out[s, r] = min over the columns c of tile s, [128 s, min(128 s + 128, n)),
    c != r, of C[r, c] (of its fp64 square if asked); NN_INF where the tile holds no other column.  Shape (ceil(n / 128), n)."""
    Cm = np.array(np.asarray(Cmat)[:n, :n], np.float64)
    assert Cm.shape == (n, n)
    if square:
        Cm = Cm * Cm
    Cm[np.arange(n), np.arange(n)] = np.inf
    slots = (n + 127) // 128
    out = np.full((slots, n), NN_INF)
    for s in range(slots):
        m = Cm[:, 128 * s:min(128 * s + 128, n)].min(axis=1)
        out[s] = np.where(np.isinf(m), NN_INF, m)
    return out


# ---- the row preparation ------------------------------------------------------------------------------------------------------------------
def row_prep_ref(src, n, p, mode):
    """linalg.hpp's row preparation of src[:n, :p] (R/get_opt_hclust.R:66-74), statistics in np.longdouble.
    mode 0: z = (x - mean) / sd with sd over p - 1, centred again as cor() does, u = c / ||c||: Cr = u, nrm = 1.
    mode 1: c = x - mean: Cr = c, nrm = ||c||; D = 1 - S read from the LOWER triangle of S and mirrored, zero diagonal (fp64).
    mode 2: D = the rows as they are with a zero diagonal (fp64); no Cr, no nrm.
    Also returned, per row: mean, sd (p - 1), A = |mean| + max |x - mean| -- what the tests' error bounds are made of."""
    x64 = np.array(np.asarray(src)[:n, :p], np.float64)
    x = x64.astype(np.longdouble)
    out = {"Cr": None, "nrm": None, "D": None}
    if mode == 2:
        assert n == p
        D = x64.copy()
        np.fill_diagonal(D, 0.0)
        out["D"] = D
        return out
    mean = x.sum(1) / p
    c = x - mean[:, None]
    sd = np.sqrt((c * c).sum(1) / max(p - 1, 1))
    out.update(mean=mean, sd=sd, A=np.abs(mean) + np.abs(c).max(1))
    if mode == 0:
        z = c / sd[:, None]
        c2 = z - (z.sum(1) / p)[:, None]
        out["Cr"] = c2 / np.sqrt((c2 * c2).sum(1))[:, None]
        out["nrm"] = np.ones(n, np.longdouble)
        return out
    assert mode == 1 and n == p
    out["Cr"] = c
    out["nrm"] = np.sqrt((c * c).sum(1))
    L = np.tril(1.0 - x64, -1)                          # one fp64 subtraction per entry, as the kernel's
    out["D"] = L + L.T
    return out


def row_prep_bounds(ref, p, mode):
    """Element-wise bounds on |computed - row_prep_ref| for fp64 arithmetic in ANY summation order: (tolerance of Cr as an (n, 1)
    column, tolerance of nrm as (n,)).  Derived in tests/test_linalg_gpu.py's docstring; first order in p u, u = 2^-53."""
    u = np.longdouble(EPS53)
    A, sd = ref["A"], ref["sd"]
    f = np.sqrt(np.longdouble(p) / max(p - 1, 1))
    if mode == 1:
        nr = ref["nrm"]
        tol_c = (p + 1) * u * A
        return tol_c[:, None], np.sqrt(np.longdouble(p)) * p * u * A + (p / 2 + 3) * u * nr + u * nr
    assert mode == 0
    kappa = A / sd                                      # the conditioning (|mean| + max |x - mean|) / sd
    zmax = (A - np.abs(ref["mean"])) / sd
    rho = f * p * u * kappa + (p / 2 + 4) * u           # sd, relative
    ez = p * u * kappa + zmax * (rho + 2 * u)           # z, absolute
    e2 = 2 * ez + (p + zmax) * u                        # z - mean2, absolute
    rho_n = f * e2 + (p / 2 + 2) * u                    # ||c||, relative
    tol = e2 / np.sqrt(np.longdouble(max(p - 1, 1))) + rho_n + 2 * u
    return tol[:, None], np.zeros(len(A), np.longdouble)    # nrm is the constant 1: exact


def row_prep_fp64(src, n, p, mode):
    """the same formulas in plain fp64 numpy with ANOTHER summation order than the kernels' (sequential, left to right): what the CPU
    test holds against row_prep_ref to show that the bounds hold for fp64 arithmetic as such"""
    x = np.array(np.asarray(src)[:n, :p], np.float64)

    def seq(a):
        return np.cumsum(a, axis=1)[:, -1]

    mean = seq(x) / p
    c = x - mean[:, None]
    if mode == 1:
        return c, np.sqrt(seq(c * c))
    sd = np.sqrt(seq(c * c) / max(p - 1, 1))
    z = c / sd[:, None]
    c2 = z - (seq(z) / p)[:, None]
    return c2 / np.sqrt(seq(c2 * c2))[:, None], np.ones(n)


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(1, 1, 1), (16, 16, 4), (63, 65, 17), (127, 129, 15), (128, 128, 16), (129, 257, 33), (300, 513, 474)]
SYM_SIZES = [1, 2, 5, 127, 128, 129, 200, 257, 385]
NN_SIZES = [2, 5, 127, 128, 129, 200, 257, 385, 2048]
NN_K = 30
EPI_CASES = [(5, 5, 47), (129, 129, 47), (200, 200, 60), (385, 385, 47), (130, 257, 47)]        # (M, N, K); M == N: also run symmetric
ROW_SHAPES = [(1, 3), (15, 30), (16, 64), (17, 65), (129, 474), (200, 512), (200, 513), (40, 1030)]
SIM_SIZES = [5, 150, 513]
DIST_SIZES = [5, 97, 300]


def int_operand(seed, K, M):
    """integers in [-8, 8] (int64): with K <= 474 every partial sum of a product is an integer below 474 * 64 < 2^53 in any order"""
    return np.random.default_rng([seed, K, M]).integers(-8, 9, size=(K, M))


def eighths_operands(seed, K, M, N):
    """(At, Bt, same) with entries m / 8, m an integer in [-3, 3]: every product is a multiple of 1/64 and every sum of K <= 474 of them,
    1 - v, the clamps and v * v are exact in fp64.  Column 1 of Bt is column 0 of At and column 2 its negative, so that (K >= 47) the
    reference holds off-diagonal entries clamped at +1 and at -1.  M == N: Bt is At with those columns, for the symmetric runs."""
    rng = np.random.default_rng([seed, K, M, N])
    At = rng.integers(-3, 4, size=(K, M)) / 8.0
    if M == N:
        At[:, 1] = At[:, 0]
        At[:, 2] = -At[:, 0]
        return At, At.copy(), True
    Bt = rng.integers(-3, 4, size=(K, N)) / 8.0
    Bt[:, 1] = At[:, 0]
    Bt[:, 2] = -At[:, 0]
    return At, Bt, False


def nn_exact_operand(seed, n, K=NN_K):
    """entries m / 8, m in [-3, 3], four in five of them zero: exact as eighths_operands, and no two columns reach a product of 1 (asserted
    on the CPU), so every distance 1 - v off the diagonal is positive"""
    rng = np.random.default_rng([seed, n, K])
    return rng.integers(-3, 4, size=(K, n)) * (rng.random((K, n)) < 0.2) / 8.0


def unit_columns(seed, K, n):
    """centred unit columns: U^T U is a correlation matrix"""
    U = np.random.default_rng([seed, K, n]).standard_normal((K, n))
    U -= U.mean(0)
    return U / np.linalg.norm(U, axis=0)


def feature_rows(seed, n, p, lds):
    """(n, lds) rows with their own location and scale, the mean within a few sd of zero; the columns beyond p hold a large junk value
    that no kernel may read into a statistic"""
    rng = np.random.default_rng([seed, n, p])
    sd = rng.uniform(0.5, 20.0, size=(n, 1))
    X = np.full((n, lds), 1.0e6)
    X[:, :p] = sd * (rng.uniform(-2.0, 2.0, size=(n, 1)) + rng.standard_normal((n, p)))
    return X


def similarity(seed, n):
    """a symmetric similarity in [0, 1] with a unit diagonal whose strict UPPER triangle is then perturbed: as.dist(1 - S) reads the lower
    one (R/get_opt_hclust.R:66-69), and a kernel that read the upper one would differ in the second digit"""
    rng = np.random.default_rng([seed, n])
    S = rng.uniform(0.0, 1.0, size=(n, n))
    S = np.tril(S, -1)
    S = S + S.T + np.eye(n)
    return S + np.triu(rng.uniform(0.01, 0.05, size=(n, n)), 1)


def distances(seed, n):
    """a symmetric distance matrix whose diagonal is NOT zero: mode 2 has to write the zeros itself"""
    rng = np.random.default_rng([seed, n])
    D = np.tril(rng.uniform(0.1, 2.0, size=(n, n)), -1)
    return D + D.T + np.diag(rng.uniform(0.5, 1.0, size=n))
