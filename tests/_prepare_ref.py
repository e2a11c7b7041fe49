"""Reference of the input preparation stage (DESIGN.md §10 "Input": PCA, then normalisation), the exact designs of
tests/test_prepare_gpu.py and its error bounds.  Test infrastructure only: written from the specification, the product never imports
it and it never imports the product.

Reference.  Centre, sd and the scores in np.longdouble (64-bit significand on x86-64); the Gram matrix exactly: every column of the
centred matrix is cut into slices of SLICE_BITS significant bits against the column's largest entry, so that a product of two slices
and the sum of n of them are exact in fp64 whatever order a BLAS adds them in (2 SLICE_BITS + log2 n <= 53), and the slice products
are added up in np.longdouble.  Four slices keep 64 bits below the column's largest entry; what they drop is below 2^-63 of the
column's largest product, the unit of np.longdouble itself.  gram_direct is the plain np.longdouble product, 100 times slower at
3000 x 600; tests/test_prepare_ref_cpu.py holds one against the other.  The Gram matrix is then rounded to fp64 and solved by numpy's
eigh (LAPACK); eigenvalues descending, each vector signed so that its largest |component| is positive.

Bounds (u = 2^-53, gamma_m = m u / (1 - m u); Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., §3.1 and §3.5).
Per principal component j the error of a score out[r, j] = xc_r . v_j has these sources:
* the centred / scaled rows.  The mean is a sum of n terms (any order: gamma_n) divided by n: |d mu_c| <= gamma_{n+1} mean|x_c|.
  The sd is a sum of n squares, a division and a root: relative error gamma_{n+4} / 2 + the mean's share, below gamma_{n+6}.  An entry
  of Xc then errs by   dxc_c = gamma_{n+1} mean|x_c| / sd_c + gamma_{n+8} |xc|   (centring and scaling; the first term only when
  centred, sd_c = 1 unscaled).  The constant part shifts a whole column: it moves the scores by sum_c shift_c |v_cj| and the Gram
  matrix by n shift shift^T + (cross terms with the column sums of Xc, which are themselves of size n shift_c).
* the Gram matrix: its accumulation gamma_n, on entries already off by gamma_{n+8} |xc| each (twice): gamma_{3n+16} |Xc|^T |Xc|, in
  the 2-norm, plus 3 n ||shift||^2.
* the solver: tests/test_eigen_cpu.py's residual bound in the Frobenius norm, ||G V - V W||_F <= c d u ||G||_F, is a backward error
  E = -(G V - V W) V^T of 2-norm at most that.  The reference's eigh carries one of its own: twice.  Rounding the reference
  Gram matrix to fp64: d u ||G||_2 at most.
* Davis-Kahan in the form of Yu, Wang & Samworth (Biometrika 102, 2015, Corollary 1): ||v^_j - v_j||_2 <= 2^(3/2) ||E||_2 / gap_j,
  gap_j = min(l_{j-1} - l_j, l_j - l_{j+1}).
* the projection: gamma_d |xc_r| . |v_j| (any order).
So   |out[r, j] - ref[r, j]| <= SAFETY ( ||xc_r||_2 2^(3/2) ||E||_2 / gap_j + gamma_{d+n+8} |xc_r| . |v_j| + shift . |v_j| ).
SAFETY = 2 covers what is second order above (products of two of these errors) and the rounding of the reference's own scores to
fp64; the issue allows up to 8.  Normalisation divides by the largest |entry| m after subtracting the column means: the same bound
over m, plus gamma_{n+1} of the column's mean |score| and 3 u."""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SAFETY = 2.0
SLICE_BITS = 16
# test_eigen_cpu.py's constant, derived there: c = 2 lambda^2 sqrt(c') + 3 * 2 * 6 sqrt(2), lambda = 4, c' = 2
C_EIGEN = 2.0 * 4.0 ** 2 * math.sqrt(2.0) + 3.0 * 2.0 * 6.0 * math.sqrt(2.0)


def gamma(m):
    return m * U / (1.0 - m * U)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def centre_scale(X, center, scale):
    """(Xc, mu, sd) in np.longdouble; sd: the divisor n - 1 about the centre used (the mean, or zero without centring)"""
    Xl = np.asarray(X, np.float64).astype(LD)
    n = Xl.shape[0]
    mu = Xl.sum(0) / LD(n) if center else np.zeros(Xl.shape[1], LD)
    Xc = Xl - mu
    sd = np.sqrt((Xc * Xc).sum(0) / LD(max(n - 1, 1))) if scale else np.ones(Xl.shape[1], LD)
    return Xc / sd, mu, sd


def gram_direct(Xc):
    return Xc.T @ Xc


def gram_sliced(Xc, slices=4):
    n, d = Xc.shape
    assert 2 * SLICE_BITS + math.ceil(math.log2(max(n, 2))) <= 53
    top = np.abs(Xc).max(0)
    e = np.where(top > 0, np.ceil(np.log2(np.where(top > 0, top, 1).astype(np.float64))) + 1, 0.0)
    rest = Xc.copy()
    S = []
    for s in range(slices):
        q = np.exp2(e - (s + 1) * SLICE_BITS).astype(LD)            # the slice's unit per column; |slice| <= 2^SLICE_BITS units
        sl = np.rint(rest / q) * q
        rest = rest - sl
        S.append(sl.astype(np.float64))
        assert np.array_equal(S[-1].astype(LD), sl)
    G = np.zeros((d, d), LD)
    for a in range(slices):
        for b in range(slices):
            G += (S[a].T @ S[b]).astype(LD)
    return G


def sign_rule(V):
    arg = np.abs(V).argmax(0)
    return V * np.where(V[arg, np.arange(V.shape[1])] < 0, -1.0, 1.0)


def pca(X, k, center=True, scale=False):
    """the reference PCA: dict with the scores (n x k, longdouble), V (d x k), every eigenvalue descending, Xc, mu, sd"""
    Xc, mu, sd = centre_scale(X, center, scale)
    G = gram_sliced(Xc).astype(np.float64)
    w, V = np.linalg.eigh((G + G.T) / 2)
    o = np.argsort(-w, kind="stable")
    k = min(k, Xc.shape[1])
    Vk = sign_rule(V[:, o[:k]])
    return {"scores": Xc @ Vk.astype(LD), "V": Vk, "w": w[o], "Xc": Xc, "mu": mu, "sd": sd, "G": G}


def normalize(S):
    S = np.asarray(S).astype(LD)
    S = S - S.sum(0) / LD(S.shape[0])
    return S / np.abs(S).max()


# ---- the bound ---------------------------------------------------------------------------------------------------------------------
def pca_bound(X, R, center, scale):
    """(bound (n x k) on |out - R["scores"]|, dict of its parts), see the module's text"""
    X = np.asarray(X, np.float64)
    n, d = X.shape
    Xc = np.abs(R["Xc"].astype(np.float64))
    V = np.abs(R["V"])
    w = R["w"]
    k = V.shape[1]
    sd = R["sd"].astype(np.float64)
    shift = gamma(n + 1) * np.abs(X).mean(0) / sd if center else np.zeros(d)
    absgram = np.linalg.norm(Xc.T @ Xc, 2)
    g2 = max(abs(w[0]), abs(w[-1]))
    e_gram = gamma(3 * n + 16) * absgram + 3 * n * float(shift @ shift)
    e_solver = 2 * C_EIGEN * d * U * float(np.linalg.norm(w)) + d * U * g2
    E = e_gram + e_solver
    gap = np.empty(k)
    for j in range(k):
        up = w[j - 1] - w[j] if j > 0 else np.inf
        dn = w[j] - w[j + 1] if j + 1 < d else np.inf
        gap[j] = min(up, dn)
    with np.errstate(divide="ignore"):
        dv = np.minimum(2.0 ** 1.5 * E / gap, 2.0)                  # (two unit vectors differ by 2 at most)
    rown = np.sqrt((Xc * Xc).sum(1))
    b = SAFETY * (rown[:, None] * dv[None, :] + gamma(d + n + 8) * (Xc @ V) + (shift @ V)[None, :])
    return b, {"E": E, "e_gram": e_gram, "e_solver": e_solver, "gap": gap, "dv": dv, "g2": g2}


def normalize_bound(S, b):
    """bound on |normalised out - normalize(S)| given |out - S| <= b entrywise"""
    S = np.asarray(S).astype(np.float64)
    n = S.shape[0]
    Sc = S - S.mean(0)
    m = np.abs(Sc).max()
    bc = b + b.mean(0)[None, :] + gamma(n + 1) * np.abs(S).mean(0)[None, :] + 3 * U * np.abs(Sc)
    # the largest |entry| errs by at most max(bc): first order in the quotient
    return (bc + np.abs(Sc) / m * bc.max()) / m * (1 + 4 * bc.max() / m)


def relative_gaps(w, k):
    """(l_j - l_{j+1}) / l_j of the first min(k + 1, d) eigenvalues"""
    m = min(k + 1, len(w))
    return (w[: m - 1] - w[1:m]) / w[: m - 1] if m > 1 else np.array([np.inf])


def zero_bound(R, parts, n, d, j):
    """bound on |out[r, j]| for a component j past the rank: out_j = Xc v^_j and ||Xc v^_j||^2 = v^_j^T (G^ + dG) v^_j
    <= |l_j| + 2 ||E||, so every entry is within the root of that (an error E in G moves a null vector's image by sqrt(E), not E)"""
    return math.sqrt(SAFETY * (abs(R["w"][j]) + 2 * parts["E"])) * (1 + gamma(d + n + 8))


def spectrum_data(n, d, lead, seed, rho=0.9, equal_pair=False):
    """n x d data whose centred Gram matrix is Q diag(l) Q^T up to rounding: l_j = n rho^j for j < lead, then n rho^lead times a
    uniform draw from [0.3, 0.9]; rank min(n - 1, d); with equal_pair l_0 = l_1.  A column mean of order 1 is added."""
    rng = np.random.default_rng(seed)
    r = min(n - 1, d)
    Z = rng.normal(size=(n, r))
    Z, _ = np.linalg.qr(Z - Z.mean(0))
    lead = min(lead, r)
    lam = np.concatenate([rho ** np.arange(lead), rho ** lead * rng.uniform(0.3, 0.9, r - lead)])
    if equal_pair:
        lam[1] = lam[0]
    Q, _ = np.linalg.qr(rng.normal(size=(d, d)))
    return (Z * np.sqrt(n * lam)) @ Q[:, :r].T + 0.5 * rng.normal(size=d)


# ---- the exact design --------------------------------------------------------------------------------------------------------------
def design_offsets(d):
    return (5 * (np.arange(d) % 7 - 3)).astype(np.float64)


def design(n, d, offsets):
    """row i < n // 2: +a_c in column c = i % d, a_c = 3 c + 4; row n // 2 + i: its negation; an odd n adds a zero row; with offsets
    o_c = 5 (c % 7 - 3) is added to column c.  Returns (X, o)."""
    h = n // 2
    X = np.zeros((n, d))
    i = np.arange(h)
    c = i % d
    X[i, c] = 3.0 * c + 4.0
    X[h + i, c] = -(3.0 * c + 4.0)
    o = design_offsets(d) if offsets else np.zeros(d)
    return X + o, o


def dense_pairs(n, d, seed):
    """a dense integer part built from +- pairs: rows 2 i and 2 i + 1 are b_i and -b_i (|entries| <= 9), an odd n adds a zero row"""
    B = np.random.default_rng(seed).integers(-9, 10, size=(n // 2, d)).astype(np.float64)
    D = np.zeros((n, d))
    D[0:2 * (n // 2):2] = B
    D[1:2 * (n // 2):2] = -B
    return D


def check_design(X, o, center):
    """what the exact cases rest on, asserted on the reference: integer data, an exact mean, an exactly diagonal Gram matrix with
    distinct non-zero integers on the used part of its diagonal.  Returns (Xc (fp64, exact), diagonal)."""
    n, d = X.shape
    assert np.array_equal(X, np.rint(X)) and np.abs(X).sum(0).max() < 2.0 ** 53
    Xl = X.astype(LD)
    s = Xl.sum(0)
    assert np.array_equal(s, (LD(n) * o.astype(LD)))                # the mean is o_c exactly, in any summation order
    Xc = X - o if center else X
    if not center:
        assert not o.any()
    G = gram_direct(Xc.astype(LD))
    dg = np.diag(G).copy()
    assert np.array_equal(G, np.diag(dg)), "the Gram matrix is exactly diagonal"
    assert dg.max() < 2.0 ** 53 and np.array_equal(dg, np.rint(dg))
    return Xc, dg.astype(np.float64)


def design_expected(Xc, dg, k):
    """the PCA of an exactly diagonal Gram matrix with k distinct leading entries: those columns of Xc, descending, unchanged"""
    o = np.argsort(-dg, kind="stable")
    k = min(k, Xc.shape[1])
    lead = dg[o[: min(k + 1, len(o))]]
    assert np.all(np.diff(lead) < 0), "the leading diagonal entries are distinct"
    assert np.all(dg[o[:k]] > 0)
    return np.ascontiguousarray(Xc[:, o[:k]])
