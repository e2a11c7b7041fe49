"""The host eigensolver (tred2 / tql2 in csrc/prepare.hip, `symmetric_eigen`) through sharp_symmetric_eigen: no device is needed.
It is the PCA's solver and the Rayleigh-Ritz step of expression_pca and of diffmap.

Bounds.  u = 2^-53.  Three assertions, each of the form  error <= c d u ||A||_2  (the orthogonality one without ||A||_2):
  ||A V - V diag(w)||_max,   ||V^T V - I||_max,   max |w - eigh(A)|.
c is derived here and not fitted to what the solver gives.  The statements below bound every column of the backward error against
the same column of A, so they are statements in the Frobenius norm as well, and a fourth assertion holds the solver to that form,
which tests/_prepare_ref.py builds on:   ||A V - V diag(w)||_F <= c d u ||A||_F.

* Tridiagonalisation.  Higham, Accuracy and Stability of Numerical Algorithms (2nd ed.), Lemma 19.3: r Householder reflectors of
  length <= m applied to A give Q^T (A + dA) with ||dA_j||_2 <= r gamma~_m ||a_j||_2 per column, gamma~_m = c' m u, c' a small
  integer (the reflector's inner product, its scaling and the update: c' = 2 covers m + 10 operations for every m >= 10, and the
  bound is not sharp below).  tred2 applies r = d - 2 reflectors from both sides: 2 (d - 2) gamma~_d, quadratic in d.  That is the
  worst case, every rounding error of one sign.  Higham & Mary (SIAM J. Sci. Comput. 41, 2019, Theorem 3.1) replace gamma_m by
  lambda sqrt(m) u for rounding errors that are independent with mean zero, failing with probability <= 2 exp(-lambda^2 / 2) by
  Hoeffding's inequality; the same argument over the r steps gives lambda sqrt(r).  Together
      2 lambda^2 sqrt(c' d) sqrt(d) u = C_TRI d u,   C_TRI = 2 lambda^2 sqrt(c'),   lambda = 4  (2 exp(-8) = 7e-4 per sum, a bound that
  real roundings, of standard deviation u / sqrt(12) and not u, stay far inside).
* QL.  A sweep is a chain of plane rotations (i, i + 1); a column of V, and a row / column of T, is touched by two of them.  Higham,
  Lemma 19.7 / 19.8: a computed rotation applied to a vector errs by at most sqrt(2) gamma_6 relative to its norm.  Golub & Van Loan,
  Matrix Computations (4th ed.) §8.3.5: about two iterations per eigenvalue (Numerical Recipes: 1.3 - 1.6); 3 is used.  Linear
  accumulation over 3 d sweeps, no probabilistic step:   C_QL = 3 * 2 * 6 sqrt(2).
* c = C_TRI + C_QL ~ 96.2.  numpy's eigh (LAPACK, the same class of method) carries an error of its own of the same form; the
  eigenvalue comparison uses the one bound for the sum of both, which the observed ratios (printed) leave room for.

A wrong rotation, a wrong deflation test or a lost Householder update shows as an error of order ||A||, 1e12 times these bounds."""
import ctypes as C
import math

import numpy as np
import pytest

U = 2.0 ** -53
LAMBDA, C_PRIME, ITER_PER_EIG = 4.0, 2.0, 3.0
C_TRI = 2.0 * LAMBDA ** 2 * math.sqrt(C_PRIME)
C_QL = ITER_PER_EIG * 2.0 * 6.0 * math.sqrt(2.0)
CC = C_TRI + C_QL
LD = np.longdouble


def eigen(A):
    """(status, w, V) of sharp_symmetric_eigen"""
    from sharp_amd._lib import f64, lib

    A = np.ascontiguousarray(A, np.float64)
    d = A.shape[0]
    w, V = np.full(d, np.nan), np.full((d, d), np.nan)
    rc = lib().sharp_symmetric_eigen(d, f64(A), f64(w), f64(V))
    return rc, w, V


def _rotation(d, seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(d, d)))
    return q * np.sign(np.diag(r))


def _wilkinson(m=10):
    d = 2 * m + 1
    A = np.diag(np.abs(np.arange(-m, m + 1)).astype(float))
    A[np.arange(d - 1), np.arange(1, d)] = 1.0
    A[np.arange(1, d), np.arange(d - 1)] = 1.0
    return A


def _sym(M):
    return (M + M.T) / 2


def _matrices():
    rng = np.random.default_rng(4)
    Q6 = _rotation(6, 5)
    rep = _sym(Q6 @ np.diag([3.0, 3.0, 3.0, 1.0, -2.0, -2.0]) @ Q6.T)
    Q12 = _rotation(12, 6)
    graded = _sym(Q12 @ np.diag(10.0 ** -np.arange(12)) @ Q12.T)
    B = rng.normal(size=(100, 2))
    R = rng.normal(size=(300, 300))
    return {
        "one": np.array([[-2.5]]),
        "zero": np.zeros((7, 7)),
        "diagonal": np.diag([4.0, -1.0, 0.0, 7.5, 2.0 ** -30, 3.0, 3.0, 1e10]),
        "repeated": rep,
        "wilkinson21": _wilkinson(10),
        "graded": graded,
        "rank2_gram": B @ B.T,
        "random300": _sym(R),
    }


MATS = _matrices()


def _ratios(A, w, V):
    """observed / bound for the residual, the orthogonality and the eigenvalues"""
    d = A.shape[0]
    norm2 = np.abs(np.linalg.eigvalsh(A)).max()
    Al, Vl, wl = A.astype(LD), V.astype(LD), w.astype(LD)
    res = float(np.abs(Al @ Vl - Vl * wl[None, :]).max())
    orth = float(np.abs(Vl.T @ Vl - np.eye(d, dtype=LD)).max())
    ev = float(np.abs(w - np.linalg.eigvalsh(A)).max())
    resf = float(np.sqrt(((Al @ Vl - Vl * wl[None, :]) ** 2).sum()))
    b = CC * d * U
    if norm2 == 0.0:
        assert res == 0.0 and ev == 0.0
        return 0.0, orth / b, 0.0, 0.0
    return res / (b * norm2), orth / b, ev / (b * norm2), resf / (b * np.linalg.norm(A, "fro"))


@pytest.mark.parametrize("name", list(MATS))
def test_eigenpairs_within_the_backward_error_bound(name):
    A = MATS[name]
    assert np.array_equal(A, A.T)
    rc, w, V = eigen(A)
    assert rc == 0
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(V))
    assert np.all(np.diff(w) >= 0), "eigenvalues ascending"
    r = _ratios(A, w, V)
    print(f"eigen {name}: d = {A.shape[0]}, residual / bound = {r[0]:.3g}, orthogonality / bound = {r[1]:.3g}, "
          f"eigenvalues / bound = {r[2]:.3g}, Frobenius residual / bound = {r[3]:.3g} (c = {CC:.1f})")
    assert max(r) <= 1.0, r


def test_one_by_one_and_zero_are_exact():
    rc, w, V = eigen(MATS["one"])
    assert rc == 0 and w[0] == -2.5 and V[0, 0] == 1.0
    rc, w, V = eigen(MATS["zero"])
    assert rc == 0 and np.array_equal(w, np.zeros(7)) and np.array_equal(V, np.eye(7))


def test_exactly_diagonal_matrix_bit_for_bit():
    """tred2's scale == 0 branch leaves a diagonal matrix alone and tql2 finds every off-diagonal already zero: the diagonal comes back
    bit for bit (sorted), every vector a unit vector"""
    A = MATS["diagonal"]
    rc, w, V = eigen(A)
    assert rc == 0
    dg = np.diag(A)
    assert np.array_equal(w, np.sort(dg))
    assert np.array_equal(np.sort(V, axis=0)[:-1], np.zeros((7, 8))) and np.array_equal(V.max(0), np.ones(8))
    assert np.array_equal(dg[V.argmax(0)], w)                  # column j is the unit vector of the entry that holds w[j]
    # with distinct, already ascending entries V is the identity itself
    rc, w, V = eigen(np.diag([-3.0, 0.5, 2.0, 9.0]))
    assert rc == 0 and np.array_equal(w, [-3.0, 0.5, 2.0, 9.0]) and np.array_equal(V, np.eye(4))


def test_repeated_eigenvalue_invariant_subspace():
    """the vectors of a repeated eigenvalue are any basis of its eigenspace: compare the projectors"""
    A = MATS["repeated"]
    rc, w, V = eigen(A)
    assert rc == 0
    wr, Vr = np.linalg.eigh(A)
    b = CC * 6 * U * 3.0
    # Davis-Kahan: a backward error E turns the projector of a cluster with gap g by at most 2 ||E|| / g; gaps here are 2 and 3
    for sl in (slice(0, 2), slice(2, 3), slice(3, 6)):
        P, Pr = V[:, sl] @ V[:, sl].T, Vr[:, sl] @ Vr[:, sl].T
        err = np.abs(P - Pr).max()
        print(f"eigen repeated: projector {sl.start}:{sl.stop} differs by {err:.3g}, bound {2 * 2 * b / 2.0:.3g}")
        assert err <= 2 * 2 * b / 2.0                          # (both solvers' errors, gap >= 2)
    assert np.abs(w - wr).max() <= b


def test_wilkinson_pairs_are_resolved():
    """W21+'s largest pair differs by about 7e-14: the values agree with LAPACK's within the bound (no relative accuracy claimed)"""
    rc, w, _ = eigen(MATS["wilkinson21"])
    assert rc == 0
    wr = np.linalg.eigvalsh(MATS["wilkinson21"])
    assert abs(w[-1] - 10.746194182903393) <= CC * 21 * U * 10.75
    assert np.abs(w - wr).max() <= CC * 21 * U * 10.75


def test_nan_is_refused_not_returned():
    """a NaN keeps the QL iteration from meeting its stop test: 60 iterations, then the refusal the PCA passes on by the caller's name"""
    from sharp_amd._lib import lib

    A = MATS["repeated"].copy()
    A[2, 1] = A[1, 2] = np.nan
    rc, _, _ = eigen(A)
    assert rc != 0
    assert b"did not converge" in lib().sharp_last_error()
    rc, w, V = eigen(MATS["repeated"])                         # the library is still usable
    assert rc == 0 and max(_ratios(MATS["repeated"], w, V)) <= 1.0


def test_bad_arguments_are_refused():
    from sharp_amd._lib import lib

    w = np.zeros(1)
    assert lib().sharp_symmetric_eigen(0, w.ctypes.data, w.ctypes.data, w.ctypes.data) != 0
    assert lib().sharp_symmetric_eigen(1, None, w.ctypes.data, w.ctypes.data) != 0
    assert b"sharp_symmetric_eigen" in lib().sharp_last_error()
